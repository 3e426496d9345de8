#!/usr/bin/env python
"""gelu_tanh_fast against its float64 definition on all 65536 fp16 inputs, measured on the GPU -> profiles/gelu_float64.txt:

    python tools/gelu_float64.py > profiles/gelu_float64.txt

The worst |out - reference| / bound (tests/gelu_model.py) of every instantiation tests/test_gpu_gelu.py runs, and of torch's
F.gelu(approximate="tanh") on the same device; how many inputs each misses the correctly rounded fp16 value on and by how much;
and the inputs on which the kernel and torch differ.  Measured values: the tests fix none of them beyond ratio <= 1.
The header names the commit: `git rev-parse`, or FPQ_GIT_HEAD where the tree is no git checkout."""
import hashlib
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

from fpqvar_amd import _lib  # noqa: E402
from tests import gelu_model as gm  # noqa: E402
from tests import test_gpu_gelu as tg  # noqa: E402


def main() -> int:
    dev = torch.device("cuda:0")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(__file__)).stdout.strip()
    except OSError:
        commit = ""
    commit = commit or os.environ.get("FPQ_GIT_HEAD", "")
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(f"# tools/gelu_float64.py: commit {commit or 'unknown (no .git here: set FPQ_GIT_HEAD)'}, libfpq_hip.so sha256 {sha}, "
          f"build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    print("# gelu_tanh_fast (fpqvar_amd/csrc/fpq_fast16.h) on all 65536 fp16 inputs against tests/gelu_model.py: reference = the float64 definition,")
    print("# bound = 1.001 ulp16(g) / 2 + 1.5 * 2^-24 |x| + 2^-22 |g| (derived from torch's fp32 op sequence).  ratio = |out - reference| / bound.")
    saved = _lib.get_option("FPQ_GEMM_CFG")
    tables = {}
    try:
        for name, run in tg.INSTANTIATIONS.items():
            x, h = run(dev, _lib.set_option)
            torch.cuda.synchronize()
            tables[name] = (x.cpu(), h.cpu())
    finally:
        _lib.set_option("FPQ_GEMM_CFG", saved)
    report(tables, Fn.gelu(gm.every_fp16(dev), approximate="tanh").cpu())
    return 0


def report(tables, ref_gpu) -> None:
    """tables: name -> (inputs, results) of every instantiation; ref_gpu: torch's results on the device"""
    every = gm.every_fp16()
    print("#\n# instantiation                                          worst ratio   at x              class mismatches")
    for name, (x, h) in list(tables.items()) + [("torch F.gelu(approximate='tanh') on this GPU", (every, ref_gpu))]:
        r = gm.ratios(h, x)
        i = int(r.argmax())
        print(f"{name:<55} {float(r[i]):10.4f}   {float(x[i]):<17.8g} {int(gm.class_mismatch(h, x).sum())}")

    first = next(iter(tg.EPILOGUE))

    def canonical(h):                         # every NaN one value, the entry of input -0 left out
        b = torch.where(torch.isnan(h), torch.full((65536,), 0x7E00), gm.bits(h))
        b[tg.NEG_ZERO] = 0
        return b

    same = all(torch.equal(canonical(h), canonical(tables[first][1])) for _, h in tables.values())
    print(f"#\n# all {len(tables)} instantiations the same bits (every NaN one value; the entry of input -0 apart): {'yes' if same else 'NO'}")
    print("# gelu(-0): " + ", ".join(sorted({f"{'stand-alone' if n in tg.STAND_ALONE else 'epilogue (sees +0)'} {float(h[tg.NEG_ZERO])!r}" for n, (_, h) in tables.items()})))

    # the kernel's one table (the stand-alone kernel: it sees -0 too) and torch's, against the correctly rounded value
    kernel = tables[next(iter(tg.STAND_ALONE))][1]
    g = gm.reference(every)
    fin = torch.isfinite(g)
    cr = gm.correctly_rounded(every)
    print("#\n# against the correctly rounded fp16 of the float64 value (finite inputs):")
    print("#                     inputs missed   largest miss [fp16 ulps of g]   at x         out            correctly rounded")
    for what, out in (("kernel", kernel), ("torch on this GPU", ref_gpu)):
        miss = fin & (gm.bits(out) != gm.bits(cr))
        ulps = torch.where(fin, (out.double() - g).abs() / gm.ulp16(g), torch.zeros_like(g))
        i = int(ulps.argmax())
        print(f"{what:<20} {int(miss.sum()):10d}   {float(ulps[i]):12.3f}                    {float(every[i]):<12.8g} {float(out[i]):<14.8g} {float(cr[i]):.8g}"
              f"      (missed with g < 0: {int((miss & (g < 0)).sum())}, with g > 0: {int((miss & (g > 0)).sum())})")

    both_nan = torch.isnan(kernel) & torch.isnan(ref_gpu)
    diff = (gm.bits(kernel) != gm.bits(ref_gpu)) & ~both_nan
    order = lambda h: torch.where(gm.bits(h) >= 0x8000, 0x8000 - gm.bits(h), gm.bits(h))
    print(f"#\n# inputs on which the kernel and torch on this GPU differ: {int(diff.sum())}")
    print("# x              kernel           torch            correctly rounded   ulps apart")
    for i in diff.nonzero().view(-1).tolist():
        print(f"{float(every[i]):<16.8g} {float(kernel[i]):<16.8g} {float(ref_gpu[i]):<16.8g} {float(cr[i]):<19.8g} {int((order(kernel) - order(ref_gpu)).abs()[i])}")


if __name__ == "__main__":
    sys.exit(main())
