#!/usr/bin/env python3
"""A/B of the format search's fused form with and without the matrix cores, on one GPU, in ONE process, alternating after warm-up:

  (f)  format_search.search_layer(xs, w, formats, fused=True)                      fake-quantized operands, torch's fp16 GEMM per weight
                                                                                  format, the products written and read by fpq_sqerr_rows_weighted
  (m)  format_search.search_layer(xs, w, formats, fused=True, matrix_cores=True)   operand codes, one GEMM-with-loss call per pair
                                                                                  (gemm.linear_*_sqerr), no product written

on one d30 mat_qkv layer at BASELINE config 4's size (100 samples, 13 600 rows, w [5760 x 1920] fp16), FP4 3 x 3 and FP6 2 x 2; the
30-layer loop with its single read-back (search_layers_fused); the largest relative difference of the two loss tables and the
winners; and a split of both forms into their stages - quantizers, reference GEMM, candidate products / loss GEMMs - each stage
timed on its own.  Every figure is device-event time around work that ends in a synchronise; every form is timed in several
bursts and its own spread (max - min over its bursts, the A/A figure) is printed beside it.

    python tools/ab_format_search_mc.py [--quick] [--out FILE] [--commit LABEL]
"""
import argparse
import hashlib
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from ab_format_search import alternate, config4_layer  # noqa: E402
from fpqvar_amd import _lib, format_search as fs, ops  # noqa: E402


def line(label, res, emit):
    mf, mm = min(res["f"]), min(res["m"])
    sf, sm = max(res["f"]) - mf, max(res["m"]) - mm
    gap, spread = mf - mm, max(sf, sm)
    verdict = "matrix cores ahead" if gap > spread else "matrix cores behind" if -gap > spread else "inside the spread"
    emit(f"{label:<34} {mf:9.3f} {sf:7.3f} {mm:9.3f} {sm:7.3f} {mf / mm:7.2f}x   {verdict}")
    emit(f"{'':<34} bursts (f) {' '.join(f'{v:.3f}' for v in res['f'])} | (m) {' '.join(f'{v:.3f}' for v in res['m'])}")


def stages(xs, w, formats, reps, bursts, emit):
    """each stage of both forms on its own: ms per layer (best burst) and its spread"""
    nf = len(formats)
    c, outs = w.shape[1], w.shape[0]
    x_all = torch.cat([x.reshape(-1, c) for x in xs])
    w_row = fs.sample_row_weights([x.numel() // c for x in xs], outs, w.device)
    ref = x_all @ w.t()
    quant = fs.quantizer
    xq = torch.cat([quant(af)(x_all) for af in formats])
    wqs = [quant(wf)(w) for wf in formats]
    ys = [(xq @ wq.t()).view(nf, x_all.shape[0], outs) for wq in wqs]
    a_ops = [fs._mc_operand(af, x_all, False) for af in formats]
    w_ops = [fs._mc_operand(wf, w, True) for wf in formats]
    table = torch.empty(nf, nf, dtype=torch.float32, device=w.device)

    def mc_losses():
        for i, wf in enumerate(formats):
            for j, af in enumerate(formats):
                fs._mc_loss(wf, af, w_ops[i], a_ops[j], ref, w_row, table[i, j])

    def fused_losses():
        for i in range(nf):
            ops.sqerr_rows_weighted(ref, ys[i], w_row, out=table[i])
    forms = {
        "reference GEMM (both)": lambda: x_all @ w.t(),
        "(f) fake-quantizers": lambda: ([quant(af)(x_all) for af in formats], [quant(wf)(w) for wf in formats]),
        f"(f) {nf} stacked fp16 GEMMs": lambda: [xq @ wq.t() for wq in wqs],
        f"(f) {nf} sqerr passes": fused_losses,
        "(m) operand quantizers": lambda: ([fs._mc_operand(af, x_all, False) for af in formats], [fs._mc_operand(wf, w, True) for wf in formats]),
        f"(m) {nf * nf} loss GEMMs": mc_losses,
    }
    res = alternate(forms, reps, bursts)
    for name, v in res.items():
        emit(f"    {name:<30} {min(v):9.3f} ms   A/A {max(v) - min(v):6.3f}")
    per_pair = min(res[f"(m) {nf * nf} loss GEMMs"]) / (nf * nf)
    flop = 2.0 * x_all.shape[0] * outs * c
    emit(f"    one loss GEMM: {per_pair * 1e3:8.1f} us, {flop / (per_pair * 1e-3) / 1e12:6.1f} TFLOP/s of its 2 T O K = {flop / 1e12:.3f} TFLOP; "
         f"one stacked fp16 GEMM per pair: {min(res[f'(f) {nf} stacked fp16 GEMMs']) / (nf * nf) * 1e3:8.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer bursts and a 6-layer loop")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--commit", default=None, help="the commit to name in the head where the tree is not a git checkout")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    commit = a.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                    cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
        except OSError:
            commit = ""
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    emit(f"# tools/ab_format_search_mc.py{' --quick' if a.quick else ''}: commit {commit or '(working tree)'}, libfpq_hip.so sha256 {sha}, "
         f"build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    emit("# ms per call (best burst) and each form's own spread over its bursts (A/A); the forms alternate burst by burst in one process")
    emit("# (f) search_layer(fused=True)   (m) search_layer(fused=True, matrix_cores=True)")
    bursts, reps = (3, 2) if a.quick else (5, 3)
    xs, w = config4_layer(dev)
    emit(f"# one d30 mat_qkv layer, {sum(x.numel() // 1920 for x in xs)} rows, w [5760 x 1920] fp16; {bursts} bursts of {reps} calls")
    emit(f"{'':<34} {'(f) ms':>9} {'A/A':>7} {'(m) ms':>9} {'A/A':>7} {'f/m':>8}")
    sets = (("FP4 3 x 3", fs.FP4_FORMATS), ("FP6 2 x 2", fs.FP6_FORMATS))
    for name, formats in sets:
        res = alternate({"f": lambda: fs.search_layer(xs, w, formats, fused=True),
                         "m": lambda: fs.search_layer(xs, w, formats, fused=True, matrix_cores=True)}, reps, bursts)
        line(f"search_layer {name}", res, emit)
    n_layers = 6 if a.quick else 30
    layers = [(xs, w)] * n_layers                      # the same tensors for every layer: one read-back per loop in both forms
    for name, formats in sets:
        def loop(mc):
            host = fs.search_layers_fused(layers, formats, matrix_cores=mc).cpu()
            return [fs.pick_winner(host[k], formats) for k in range(n_layers)]
        res = alternate({"f": lambda: loop(False), "m": lambda: loop(True)}, 1, bursts, warm=1)
        line(f"{n_layers} layers {name} (ms per loop)", res, emit)
    del layers
    emit("#")
    emit("# the two loss tables of the layer: (weight format, activation format), matrix cores against fused, relative difference")
    for name, formats in sets:
        wf_f, af_f, lf = fs.search_layer(xs, w, formats, fused=True)
        wf_m, af_m, lm = fs.search_layer(xs, w, formats, fused=True, matrix_cores=True)
        worst = max(abs(lm[k] - lf[k]) / lf[k] for k in lf)
        emit(f"{name}: winner fused {(wf_f, af_f)}, matrix cores {(wf_m, af_m)}; largest |m - f| / f over the pairs {worst:.3g}")
        for k in lf:
            emit(f"    {str(k):<28} f {lf[k]:.8g}  m {lm[k]:.8g}  rel {abs(lm[k] - lf[k]) / lf[k]:.3g}")
    emit("#")
    emit("# the stages of one layer, each timed on its own (ms per layer; the forms' sums are not their end-to-end times: torch's allocator,")
    emit("# the concatenation and the launches in between are in the end-to-end lines above only)")
    for name, formats in sets:
        emit(f"{name}:")
        stages(xs, w, formats, reps, bursts, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
