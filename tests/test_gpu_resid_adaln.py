"""GPU: the adaLN producers with the gated residual in front folded in (rotation.resid_adaln_rotate_quant / _mx / _token,
include/fpq.h fpq_resid_adaln_*).  The contract is bit equality, no tolerance anywhere:
  1. x_new is bit for bit `residual + y.mul(gate)` as torch computes it on the GPU (fp16 rows: also ops.gate_residual);
  2. every other output is byte for byte what the twin entry point returns for x_new."""
import pytest
import torch

from tests.test_gpu_adaln import MFMA_WIDTHS

pytestmark = pytest.mark.gpu

B = 3
LENGTHS = (1, 5, 37)   # an odd L ends a PAIR2 or paired-slot unit with a single row


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def same(a, b, what):
    a, b = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    assert len(a) == len(b), what
    for i, (p, q) in enumerate(zip(a, b)):
        assert p.dtype == q.dtype and p.shape == q.shape, f"{what}[{i}]: {p.dtype} {tuple(p.shape)} != {q.dtype} {tuple(q.shape)}"
        assert torch.equal(p.contiguous().view(torch.uint8), q.contiguous().view(torch.uint8)), f"{what}[{i}]: bytes differ"


def inputs(dev, C, L, row_dtype, mod_dtype, seed, b=B):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(b, L, C, generator=g).half().to(dev)
    gate = (torch.randn(b, 1, C, generator=g) * 0.5).half().to(dev)
    resid = torch.randn(b, L, C, generator=g).to(row_dtype).to(dev)
    sc = (torch.randn(b, 1, C, generator=g) * 0.3).to(mod_dtype).to(dev)
    sh = (torch.randn(b, 1, C, generator=g) * 0.3).to(mod_dtype).to(dev)
    return y, gate, resid, sc, sh


def forms(rot):
    """(name, fused call, twin call on x_new) - all four forms, both layouts where a form has two"""
    out = []
    for table in ("e2m1", "e2m3"):
        for ri in (False, True):
            out.append((f"values {table}{' +h +rotated' if ri else ''}",
                        lambda a, kw, t=table, r=ri: rot.resid_adaln_rotate_quant(*a, t, return_intermediates=r, **kw),
                        lambda x, sc, sh, kw, t=table, r=ri: rot.adaln_rotate_quant(x, sc, sh, t, return_intermediates=r, **kw)))
    for km in (False, True):
        out.append((f"FP4 operands{' k-major' if km else ''}",
                    lambda a, kw, k=km: rot.resid_adaln_rotate_quant_mx(*a, kmajor=k, **kw),
                    lambda x, sc, sh, kw, k=km: rot.adaln_rotate_quant_mx(x, sc, sh, kmajor=k, **kw)))
    for table in ("e2m3", "e3m2"):
        out.append((f"token values {table}",
                    lambda a, kw, t=table: rot.resid_adaln_rotate_quant_token(*a, t, **kw),
                    lambda x, sc, sh, kw, t=table: rot.adaln_rotate_quant_token(x, sc, sh, t, **kw)))
        for km in (False, True):
            out.append((f"token fp6 codes {table}{' k-major' if km else ''}",
                        lambda a, kw, t=table, k=km: rot.resid_adaln_rotate_quant_token(*a, t, emit="fp6", kmajor=k, **kw),
                        lambda x, sc, sh, kw, t=table, k=km: rot.adaln_rotate_quant_token(x, sc, sh, t, emit="fp6" if t == "e2m3" else "bf6",
                                                                                           kmajor=k, **kw)))
    return out


def check_all_forms(rot, ops, args, smooth, what, only=None):
    y, gate, resid, sc, sh = args
    want_x = resid + y.mul(gate)                      # torch's own two kernels; the sum takes the residual's dtype
    assert want_x.dtype is resid.dtype
    if resid.dtype is torch.float16:
        same(ops.gate_residual(y, gate, resid), want_x, what + ": ops.gate_residual against torch")
    kw = {"smooth": smooth}
    for name, fused, twin in forms(rot):
        if only is not None and not any(o in name for o in only):
            continue
        got = fused((y, gate, resid, sc, sh), kw)
        same(got[0], want_x, f"{what} {name}: x_new")
        want = twin(got[0], sc, sh, kw)
        same(tuple(got[1:]), want if isinstance(want, tuple) else (want,), f"{what} {name}")


@pytest.mark.parametrize("C", MFMA_WIDTHS)
def test_shape_sweep(dev, C, lib_options):
    """MAXC 1 .. 5, PAIR2 (1024), TIGHT (1920), the slot partly (2304) and fully (2560) used; both row dtypes, both modulation
    dtypes, with and without the smoothing vector; every workgroup cut, and the switches that choose another variant - the twin
    under the same option"""
    from fpqvar_amd import ops, rotation as rot
    sm = (torch.rand(C, generator=torch.Generator().manual_seed(C)) + 0.5).to(dev)
    cases = [(L, rd, md, s) for L in LENGTHS for rd in (torch.float16, torch.float32) for md in (torch.float16, torch.float32)
             for s in (None, sm)]
    data = {c[:3]: inputs(dev, C, c[0], c[1], c[2], 1000 * C + 7 * c[0] + (c[1] is torch.float32) + 2 * (c[2] is torch.float32)) for c in cases}
    for rows in (None, 1, 2, 3):
        lib_options("FPQ_ADALN_ROWS", rows)
        for L, rd, md, s in cases:
            check_all_forms(rot, ops, data[(L, rd, md)], s, f"C={C} L={L} rows={rd} mod={md} smooth={s is not None} FPQ_ADALN_ROWS={rows}")
    lib_options("FPQ_ADALN_ROWS", None)
    switches = [("FPQ_NO_HW4", ("values e2m1", "FP4 operands")), ("FPQ_NO_HW6", ("values e2m3", "token values"))]
    if C == 1024:
        switches.append(("FPQ_ADALN_NO_PAIR2", ("values", "FP4 operands")))
    if C == 1920:
        switches.append(("FPQ_ADALN_NO_TIGHT", ("values e2m1",)))
    for name, only in switches:
        lib_options(name, 1)
        for L, rd, md, s in cases:
            check_all_forms(rot, ops, data[(L, rd, md)], s, f"C={C} L={L} rows={rd} mod={md} smooth={s is not None} {name}=1", only)
        lib_options(name, None)


def test_large_launch_cut(dev):
    """[20 x 576 x 2304] fp16 rows into FP4 operands and into values: large launches take the cut of 8 / 12 rows per workgroup by
    themselves - the shape at which the 6-bit group producers once came out one rounding apart"""
    from fpqvar_amd import ops, rotation as rot
    g = torch.Generator(device=dev).manual_seed(5)
    b, L, C = 20, 576, 2304
    y = torch.randn(b, L, C, device=dev, generator=g).half()
    gate = (torch.randn(b, 1, C, device=dev, generator=g) * 0.5).half()
    resid = torch.randn(b, L, C, device=dev, generator=g).half()
    sc = (torch.randn(b, 1, C, device=dev, generator=g) * 0.3).half()
    sh = (torch.randn(b, 1, C, device=dev, generator=g) * 0.3).half()
    sm = torch.rand(C, device=dev, generator=g) + 0.5
    check_all_forms(rot, ops, (y, gate, resid, sc, sh), sm, "large launch", only=("FP4 operands", "values e2m1"))


@pytest.mark.parametrize("row_dtype", (torch.float16, torch.float32))
@pytest.mark.parametrize("C", (1024, 1920, 2304))
def test_special_rows(dev, C, row_dtype):
    """a NaN in y, +-inf in the residual, a product that overflows fp16, a row whose x_new is all zeros, a subnormal product: x_new is
    torch's, and what the twin makes of such an x_new is the expectation"""
    from fpqvar_amd import ops, rotation as rot
    y, gate, resid, sc, sh = inputs(dev, C, 7, row_dtype, torch.float16, 99 + C, b=2)
    gate[:, 0, 5], gate[:, 0, 9] = 300.0, 2.0 ** -3
    y[0, 0, 17] = float("nan")
    resid[0, 1, 3] = float("inf")
    resid[0, 2, C - 1] = float("-inf")
    y[0, 3, 5] = 300.0                                       # 300 * 300 overflows fp16: the product is +inf
    y[1, 3, 5] = -300.0
    resid[0, 4] = (-(y[0, 4].mul(gate[0, 0]))).to(row_dtype)  # x_new == 0 everywhere (the negated product is exact in either dtype)
    y[1, 5], resid[1, 5] = 0.0, 0.0                          # ... and with every operand zero
    y[0, 6, 9], resid[0, 6, 9] = 2.0 ** -14, 0.0             # 2^-14 * 2^-3: a subnormal fp16 product, which x_new then is
    want_x = resid + y.mul(gate)
    assert bool(torch.isnan(want_x[0, 0, 17])) and bool(torch.isinf(want_x[0, 1, 3])) and bool(torch.isinf(want_x[0, 3, 5]))
    assert not bool(want_x[0, 4].any()) and not bool(want_x[1, 5].any()) and float(want_x[0, 6, 9]) == 2.0 ** -17
    check_all_forms(rot, ops, (y, gate, resid, sc, sh), None, f"special rows C={C} {row_dtype}")


@pytest.mark.parametrize("row_dtype", (torch.float16, torch.float32))
def test_in_place(dev, row_dtype):
    """inplace=True: the same bytes as out of place, and `residual` then holds x_new (it is the tensor that comes back)"""
    from fpqvar_amd import rotation as rot
    for C in (1024, 1920, 2304):
        args = inputs(dev, C, 37, row_dtype, torch.float16, 3 * C)
        for name, fused, _ in forms(rot):
            want = fused(args, {"smooth": None})
            y, gate, resid, sc, sh = args
            r2 = resid.clone()
            got = fused((y, gate, r2, sc, sh), {"smooth": None, "inplace": True})
            assert got[0].data_ptr() == r2.data_ptr(), name
            same(tuple(got), tuple(want), f"in place C={C} {name}")
            same(r2, want[0], f"in place C={C} {name}: residual")


def test_compiled_binding_equals_ctypes_path(dev, monkeypatch):
    """the four forms through the compiled binding against the same calls through ctypes (the wrappers with `_native` taken away)"""
    from fpqvar_amd import _native, rotation as rot
    assert rot._native is _native
    for row_dtype in (torch.float16, torch.float32):
        args = inputs(dev, 1920, 37, row_dtype, torch.float16, 11, b=4)
        sm = (torch.rand(1920, generator=torch.Generator().manual_seed(3)) + 0.5).to(dev)
        for smooth in (None, sm):
            for name, fused, _ in forms(rot):
                if "+h" in name:
                    continue   # the emitting form has no compiled binding, as its twin has none
                for inplace in (False, True):
                    a = fused((*args[:2], args[2].clone(), *args[3:]), {"smooth": smooth, "inplace": inplace})
                    with monkeypatch.context() as m:
                        m.setattr(rot, "_native", None)
                        b = fused((*args[:2], args[2].clone(), *args[3:]), {"smooth": smooth, "inplace": inplace})
                    same(tuple(a), tuple(b), f"native against ctypes: {name} {row_dtype} inplace={inplace}")


def test_captured_graph(dev):
    """three replays with changed inputs, each equal to the eager call"""
    from fpqvar_amd import rotation as rot
    C, L = 2304, 37
    static = [t.clone() for t in inputs(dev, C, L, torch.float32, torch.float16, 1)]
    calls = [lambda a: rot.resid_adaln_rotate_quant_mx(*a, kmajor=True),
             lambda a: rot.resid_adaln_rotate_quant_token(*a, "e2m3", emit="fp6"),
             lambda a: rot.resid_adaln_rotate_quant(*a, "e2m1")]
    for call in calls:
        call(static)   # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = [call(static) for call in calls]
    for rep in range(3):
        fresh = inputs(dev, C, L, torch.float32, torch.float16, 100 + rep)
        for s, f in zip(static, fresh):
            s.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        for call, out in zip(calls, outs):
            same(tuple(out), tuple(call(fresh)), f"replay {rep}")


@pytest.mark.parametrize("config", ("w4a4", "w6a6"))
def test_model_level(dev, config, monkeypatch):
    """GenerationBatch(fuse_residual=True): two scale steps (patch sizes 1 and 3) of a two-block model, bit-equal to
    fuse_residual=False on paths F and Q"""
    from fpqvar_amd import var_block
    gb = var_block.GenerationBatch(depth=2, batch_rows=4, config=config, device=dev, fuse_residual=True)
    assert gb.fuse_residual is True
    xs = [gb.new_input(pn) for pn in (1, 3)]
    calls = []
    inner = gb.resid_producer
    monkeypatch.setattr(gb, "resid_producer", lambda path, *a: calls.append(path) or inner(path, *a))
    for path in ("F", "Q"):
        got = {}
        for fuse in (False, True):
            gb.fuse_residual = fuse
            caches = gb.new_caches(path)
            calls.clear()
            got[fuse] = [gb.step(path, caches, x.clone()) for x in xs]
            # per step of two blocks - path F: proj's tail in both blocks + fc2's tail of the first; path Q: fc2's tail of the first
            assert calls == ([path] * (2 * (3 if path == "F" else 1)) if fuse else []), (path, fuse, calls)
        same(tuple(got[True]), tuple(got[False]), f"{config} path {path}")


def test_fuse_residual_is_off_by_default(dev):
    from fpqvar_amd import var_block
    import inspect
    assert inspect.signature(var_block.GenerationBatch.__init__).parameters["fuse_residual"].default is False


def test_fp4linear_adaln_operands_pending(dev):
    """FP4Linear.adaln_operands(pending=(y, gate)) against gate_residual + adaln_operands, and the product through forward_operands"""
    from fpqvar_amd import gemm, ops
    g = torch.Generator().manual_seed(21)
    C, O, L = 1920, 256, 37
    lin = torch.nn.Linear(C, O).to(dev)
    y, gate, resid, sc, sh = inputs(dev, C, L, torch.float16, torch.float16, 31)
    sm = (torch.rand(C, generator=g) + 0.5).to(dev)
    for kmajor in (False, True):
        mod = gemm.FP4Linear.from_float(lin, kmajor=kmajor)
        x_new, codes, scales = mod.adaln_operands(resid, sc, sh, smooth=sm, pending=(y, gate))
        want_x = ops.gate_residual(y, gate, resid)
        want = mod.adaln_operands(want_x, sc, sh, smooth=sm)
        same((x_new, codes, scales), (want_x, *want), f"adaln_operands(pending=) kmajor={kmajor}")
        same(mod.forward_operands(codes, scales), mod.forward_operands(*want), f"forward_operands kmajor={kmajor}")
    mod6 = gemm.FP4Linear.from_float(lin, act_fp_type="fp_e3")
    with pytest.raises(RuntimeError, match="pending= needs an 'e2m1' activation"):
        mod6.adaln_operands(resid, sc, sh, pending=(y, gate))
