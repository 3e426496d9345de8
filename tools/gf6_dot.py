#!/usr/bin/env python3
"""Does the matrix core keep every product of a 128-term dot of FULL-RANGE FP6 codes?  The measurement the GF6 contract rests on
(include/fpq.h "GF6", DESIGN.md section 4b''''), taken before any test is tuned to it - as profiles/r09_a6w4_dot.txt and
profiles/w6_dot.txt were for the E1M2 / E3M0 tables.

K = 128, unit scales, no bias, both tilings (FPQ_GEMM_CFG 20 / 30), every (activation, weight) pair with at least one E2M3 / E3M2
side through gemm.linear_g6, on the constructions of tests/gf6_model.exact_dot_cases - dots that are fp16 numbers: the largest
products cancelling beside a few smallest ones, every level pair alone and N-fold, the largest product beside 127 small ones.
A construction "came out" when every output equals the exact dot bit for bit.  The paper figures (products are multiples of `step`,
at most `largest`; the dot has at most `bits` significant bits) are printed beside each pair.
--sweep: instead, the worst error / tests/gemm_model.bound per pair over the shape sweep of tests/test_gpu_gf6.py (every family x
tokens 1, 17, 65, 130 x outs 8, 136, 384 x K 128, 384, 1920; both tilings row-major and the library's choice on k-major images),
the pairs gemm.linear_g6 refuses included - the record behind that refusal (profiles/gf6_gemm_bound.txt).
usage: gf6_dot.py > profiles/gf6_dot.txt;  gf6_dot.py --sweep > profiles/gf6_gemm_bound.txt"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fpqvar_amd import _lib, gemm  # noqa: E402
from tests import gemm_model as gm  # noqa: E402
from tests import gf6_model as fm  # noqa: E402

dev = torch.device("cuda:0")
gemm.GF6_REFUSED_PAIRS = frozenset()   # a measurement: the pairs the Python layer refuses BECAUSE of this file's result run here too
CFGS = (20, 30)


def main():
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(f"# tools/gf6_dot.py: libfpq_hip.so sha256 {sha}, build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    print("# K = 128, unit scales, no bias; per pair, tiling and construction: outputs that differ from the exact dot (an fp16 number),")
    print("# the largest |error|, that error in units of the smallest product of the pair, and against tests/gemm_model.bound")
    summary = []
    for at, wt in fm.PAIRS:
        step, largest, bits = fm.product_range(at, wt)
        print(f"\n{at} x {wt}  ({fm.FAMILY[at, wt]} family; products: multiples of 2^{int(torch.log2(torch.tensor(step)))}, at most {largest:g}; "
              f"128-term dot: at most {bits} bits)")
        exact_runs = runs = 0
        worst_pair = 0.0
        for name, (La, Lw) in fm.exact_dot_cases(at, wt).items():
            a, w = fm.encode_levels(at, La).to(dev), fm.encode_levels(wt, Lw).to(dev)
            sa = torch.ones(La.shape[0], 1, dtype=torch.float16, device=dev)
            sw = torch.ones(Lw.shape[0], 1, dtype=torch.float32, device=dev)
            exact = (La @ Lw.t()).half().to(dev)
            for cfg in CFGS:
                with _lib.option("FPQ_GEMM_CFG", cfg):
                    y = gemm.linear_g6(a, sa, at, w, sw, wt)
                torch.cuda.synchronize()
                n_bad = int((y.view(torch.int16) != exact.view(torch.int16)).sum())
                rat = gm.ratio(y, fm.reference(at, wt, a, sa, w, sw, None))
                worst = float((y.double() - exact.double()).abs().max())
                runs += 1
                exact_runs += n_bad == 0
                worst_pair = max(worst_pair, worst)
                print(f"  {name:13s} cfg {cfg}: {n_bad:5d} of {y.numel():5d} differ, max |err| {worst:<10g} = {worst / step:g} steps, err / bound {rat:.3f}", flush=True)
        summary.append((at, wt, exact_runs, runs, bits, worst_pair))
    print("\n# summary: constructions bit for bit / run, per pair")
    for at, wt, ok, runs, bits, worst in summary:
        print(f"{at} x {wt}: {ok} of {runs} exact ({bits} bits on paper; max |err| {worst:g})  {'EXACT' if ok == runs else 'NOT EXACT'}")


def sweep():
    """profiles/gf6_gemm_bound.txt"""
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(f"# tools/gf6_dot.py --sweep: libfpq_hip.so sha256 {sha}, build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    print("# worst error / tests/gemm_model.bound per (activation x weight) pair with a full FP6 side, against the float64 product of the")
    print("# decoded operands: every family of tests/gf6_model.py x tokens 1, 17, 65, 130 x outs 8, 136, 384 x K 128, 384, 1920, FPQ_GEMM_CFG 20")
    print("# and 30 on row-major operands and the library's choice on k-major images (gemm.linear_g6 with its refusal lifted).  model: every")
    print("# output bit-equal to the fp32 model of the kernel's steps; same bits: tilings and layouts bit-equal to each other.")
    print("# The contract (include/fpq.h, GF6): 1.0 where profiles/gf6_dot.txt came out bit for bit, else gemm_model.WIDE_FP8_MEASURED = 8.0;")
    print("# a pair past its allowance is refused by gemm.linear_g6*.")
    print("# pair          family  worst err / bound   model   same bits   worst family")

    def images(pair, c):
        ab, wb = (4 if pair[0] == "e2m1" else 6), (4 if pair[1] == "e2m1" else 6)
        return (gemm.to_kmajor(c["a"], ab), gemm.to_kmajor_scales(c["a_scales"]), pair[0], gemm.to_kmajor(c["w"], wb, dealt=True),
                gemm.to_kmajor_scales(c["w_scales"], weight_side=True), pair[1])
    worst = {p: (0.0, "") for p in fm.PAIRS}
    model = {p: True for p in fm.PAIRS}
    same = {p: True for p in fm.PAIRS}
    for family in fm.FAMILIES:
        for T in (1, 17, 65, 130):
            for O in (8, 136, 384):
                for K in (128, 384, 1920):
                    for pair in fm.PAIRS:
                        c = fm.make_case(*pair, family, T, O, K, device=dev)
                        args = (c["a"], c["a_scales"], c["w"], c["w_scales"], c["bias"])
                        r, emu = fm.reference(*pair, *args), fm.emulate(*pair, *args)
                        runs = []
                        for cfg in CFGS:
                            with _lib.option("FPQ_GEMM_CFG", cfg):
                                runs.append(gemm.linear_g6(c["a"], c["a_scales"], pair[0], c["w"], c["w_scales"], pair[1], c["bias"]))
                        runs.append(gemm.linear_g6(*images(pair, c), c["bias"], outs=O))
                        for y in runs:
                            rat = gm.ratio(y, r)
                            if rat > worst[pair][0]:
                                worst[pair] = (rat, family)
                            yn, en = torch.isnan(y), torch.isnan(emu)
                            model[pair] &= bool(torch.equal(yn, en)) and bool(torch.equal(y.masked_fill(yn, 0).view(torch.int16), emu.masked_fill(en, 0).view(torch.int16)))
                            same[pair] &= bool(torch.equal(y.masked_fill(yn, 0).view(torch.int16), runs[0].masked_fill(torch.isnan(runs[0]), 0).view(torch.int16)))
    for pair in fm.PAIRS:
        rat, fam = worst[pair]
        print(f"{pair[0]} x {pair[1]}   {fm.FAMILY[pair]:5s}   {rat:12.3f}        {'yes' if model[pair] else 'no ':3s}     {'yes' if same[pair] else 'no ':3s}         {fam}", flush=True)


if __name__ == "__main__":
    sweep() if "--sweep" in sys.argv[1:] else main()
