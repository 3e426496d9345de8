#!/usr/bin/env python3
"""The figures of profiles/block_step_refactor.txt for ONE source tree per process: two trees that share the libraries' bytes are
compared by running this once per tree, alternating, and diffing what it prints.

    python tools/block_step_ab.py digests [ROOT]    one sha256 per case of tests/test_gpu_block_step.py's grid (this tree's file) over every
                                                    step output and every block's cache contents of the run
    python tools/block_step_ab.py eager [ROOT]      GenerationBatch.run_eager at d30-256, depth 4, paths F and Q: best of five, ms
    python tools/block_step_ab.py bench FILE...     headline value and every generation record's ms_per_batch of bench.py's JSON lines

ROOT: the tree whose fpqvar_amd (and tests.conftest) is imported; default: the tree of this file."""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    mode, rest = sys.argv[1], sys.argv[2:]
    if mode == "bench":
        for name in rest:
            with open(name) as f:
                line = json.loads([ln for ln in f if ln.startswith("{")][-1])
            gen = " ".join(f"{r['model']}/{r['path']}={r.get('ms_per_batch', r.get('error'))}" for r in line.get("generation", []))
            print(f"{os.path.basename(name)}: value={line['value']} {line['unit']} ms_per_step={line['ms_per_step']}  ms_per_batch: {gen}")
        return
    root = os.path.abspath(rest[0]) if rest else HERE
    sys.path.insert(0, root)
    import fpqvar_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(fpqvar_amd.__file__))) == root, f"fpqvar_amd came from {fpqvar_amd.__file__}"
    if mode == "digests":
        spec = importlib.util.spec_from_file_location("block_step_cases", os.path.join(HERE, "tests", "test_gpu_block_step.py"))
        cases = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(cases)
        for case in cases.CASES:
            print(cases.case_id(case), cases.digest(case), flush=True)
    elif mode == "eager":
        from fpqvar_amd import var_block
        gb = var_block.GenerationBatch("d30-256", depth=4)
        for path in "FQ":
            gb.run_eager(path)   # allocator, kernel load
            print(f"run_eager {path}: {min(gb.run_eager(path) for _ in range(5)):.2f} ms", flush=True)
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
