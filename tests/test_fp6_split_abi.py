"""fpq_gemm_fp6_rows_split / fpq_gemm_fp6_rows_split_qknorm without a GPU: the argument checks of the C entry points return the
documented codes before anything touches a device (the pointers below are never dereferenced: every call is refused, or has no
tokens), and the new instantiations of gemm_fp6_rows_kernel keep the ISA properties of the plain ones - no scratch, no spill,
fragment reads as ds_read_b64 (fpq_gemm_fp6.h, FPQ_LDS_READ64) - read from the built library's code objects as
tests/test_no_spill.py reads them."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.test_no_spill import LIB, _code_objects, _tool, kernel_metadata

OK, ERR_ARG, ERR_DTYPE, ERR_SHAPE = 0, -1, -2, -3
F16, F32 = 0, 1   # enum fpq_dtype
PTR = 0x7000_0000_1000   # an address with every alignment the checks ask for; nothing reads it


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


def _split(part_cols=128, n_parts=3, rows_per_batch=4, out=(PTR, PTR, PTR), row_stride=None):
    from fpqvar_amd._lib import GemmSplit
    sp = GemmSplit()
    sp.part_cols, sp.n_parts, sp.rows_per_batch = part_cols, n_parts, rows_per_batch
    for p in range(3):
        sp.out[p], sp.row_stride[p], sp.batch_stride[p], sp.row0[p] = out[p], row_stride or part_cols, 16, 0
    return sp


def _call(lib, norm, sp, tokens=8, outs=None, k=128, bias=None, head_scale=PTR, a_dtype=F16, w_dtype=F32, kmajor=0, a=PTR):
    outs = sp.n_parts * sp.part_cols if outs is None else outs
    ref = ctypes.byref(sp)
    if norm:
        return lib.fpq_gemm_fp6_rows_split_qknorm(a, PTR, a_dtype, PTR, PTR, w_dtype, bias, tokens, outs, k, ref, head_scale, kmajor, None)
    return lib.fpq_gemm_fp6_rows_split(a, PTR, a_dtype, PTR, PTR, w_dtype, bias, tokens, outs, k, ref, kmajor, None)


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("kmajor", [0, 1])
def test_checks_come_before_any_launch(lib, norm, kmajor):
    def call(sp, **kw):
        return _call(lib, norm, sp, kmajor=kmajor, **kw)
    assert call(_split(), tokens=0) == OK                                   # nothing to do: no launch
    assert call(_split(rows_per_batch=3), tokens=8) == ERR_ARG              # tokens % rows_per_batch
    assert call(_split(rows_per_batch=0)) == ERR_ARG
    assert call(_split(part_cols=192)) == ERR_ARG                           # part_cols % 128
    assert call(_split(part_cols=0)) == ERR_ARG
    assert call(_split(), outs=256) == ERR_ARG                              # outs != n_parts * part_cols
    assert call(_split(n_parts=0)) == ERR_ARG
    assert call(_split(n_parts=4)) == ERR_ARG
    for p in range(3):                                                      # every destination: non-NULL, 8-byte aligned
        for bad in (None, PTR + 4, PTR + 2):
            out = [PTR, PTR, PTR]
            out[p] = bad
            assert call(_split(out=tuple(out))) == ERR_ARG, (p, bad)
    assert call(_split(row_stride=64)) == ERR_ARG                           # row_stride < part_cols
    assert call(_split(row_stride=130)) == ERR_ARG                          # row_stride % 4
    assert call(_split(out=(PTR + 8, PTR + 8, PTR + 8)), tokens=0) == OK    # 8-byte alignment is enough, for all parts
    # what fpq_gemm_fp6_rows_ex checks
    assert call(_split(), k=96) == ERR_SHAPE
    assert call(_split(), a_dtype=7) == ERR_DTYPE
    assert call(_split(), w_dtype=7) == ERR_DTYPE
    assert call(_split(), a=None) == ERR_ARG
    assert call(_split(), a=PTR + 8) == ERR_ARG                             # code arrays 16-byte aligned
    assert call(_split(), tokens=-4) == ERR_ARG
    if norm:
        assert call(_split(n_parts=2)) == ERR_ARG                           # q, k, v: exactly three parts
        assert call(_split(n_parts=1)) == ERR_ARG
        assert call(_split(), head_scale=None) == ERR_ARG
        assert call(_split(), bias=PTR + 8) == ERR_ARG                      # the fp32 bias is read 16 bytes at a time
        assert call(_split(), bias=PTR + 16, tokens=0) == OK
    else:
        assert call(_split(n_parts=2), tokens=0) == OK
        assert call(_split(n_parts=1), tokens=0) == OK


def test_null_descriptor(lib):
    assert lib.fpq_gemm_fp6_rows_split(PTR, PTR, F16, PTR, PTR, F32, None, 8, 384, 128, None, 0, None) == ERR_ARG
    assert lib.fpq_gemm_fp6_rows_split_qknorm(PTR, PTR, F16, PTR, PTR, F32, None, 8, 384, 128, None, PTR, 0, None) == ERR_ARG


def _fp6_kernels(recs):
    """{epilogue: [(name, record)]} of gemm_fp6_rows_kernel's instantiations, by the mangled name's last template argument"""
    out = {"GemmNoFc1": [], "GemmSplit": [], "GemmQkNorm": []}
    for n, r in recs:
        if "gemm_fp6_rows_kernel" in n:
            for e in out:
                if e in n:
                    out[e].append((n, r))
    return out


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfpq_hip.so not built")
def test_new_instantiations_do_not_spill(tmp_path):
    kernels = _fp6_kernels(kernel_metadata(tmp_path))
    for e in ("GemmSplit", "GemmQkNorm"):
        assert len(kernels[e]) == 8, (e, [n for n, _ in kernels[e]])       # four scale-dtype pairs x {128, 256} rows
        for n, r in kernels[e]:
            assert int(r.get("vgpr_spill_count", 0)) == 0 and int(r.get("sgpr_spill_count", 0)) == 0, (n, r)
            assert int(r.get("private_segment_fixed_size", 0)) == 0, (n, r.get("private_segment_fixed_size"))
            # two workgroups of four wavefronts per CU = two wavefronts per SIMD: 512 / 2 registers per lane
            assert int(r["vgpr_count"]) + int(r.get("agpr_count", 0)) <= 256, (n, r["vgpr_count"])


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfpq_hip.so not built")
def test_new_instantiations_read_fragments_with_ds_read_b64(tmp_path):
    checked = 0
    for elf in _code_objects(tmp_path):
        txt = subprocess.run([_tool("llvm-objdump"), "-d", "--no-show-raw-insn", elf], capture_output=True, text=True, check=True).stdout
        for block in re.split(r"\n(?=[0-9a-fA-F]+ <)", txt):
            head = block.split("\n", 1)[0]
            if "gemm_fp6_rows_kernel" not in head or not ("GemmSplit" in head or "GemmQkNorm" in head):
                continue
            ops = [l.split()[0] for l in block.splitlines()[1:] if l.strip()]
            per_step = 3 * (4 + (8 if "Li8ELi4E" in head else 4))          # three 8-byte pieces per fragment, NT + MT fragments
            assert ops.count("ds_read_b64") == per_step, (head, ops.count("ds_read_b64"))
            assert not [o for o in ops if o.startswith("ds_read2")], head
            assert not [o for o in ops if o.startswith("scratch_")], head
            assert [o for o in ops if o.startswith("v_mfma")], head
            checked += 1
    assert checked == 16, checked
