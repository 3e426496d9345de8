"""The Python front of the row producers (rotation.rotate_quant*, adaln_rotate_quant*, resid_adaln_rotate_quant*) without a GPU, in the
manner of tests/test_linear_call_path_host.py: which C entry point each of the twelve public functions ends in, every argument it
passes, what it returns and every refusal, with the library replaced by a recorder.  CPU tensors stand in for the operands - nothing
reads them; a pointer is told by the tensor it belongs to (`retN`: the N-th tensor the call returned, `tmpN`: anything else the call
allocated - a contiguous copy of x, modulation rows, a converted smooth vector)."""
import contextlib
import ctypes

import pytest
import torch

from fpqvar_amd import _lib, rotation as rot

F16, F32 = 0, 1
C, G, ROWS, PAD = 256, 2, 6, 8                       # two 128-groups; six rows, so two padded columns in a k-major scale image
TID = _lib.TABLE_IDS
f16, f32, u8 = torch.float16, torch.float32, torch.uint8
MASK0 = tuple(rot.sign_mask(rot.sign_vector(128, 42)))
D = torch.ones(128)
D[::3] = -1.0
MASKD = tuple(rot.sign_mask(D))
SIGNS = {"default": (None, MASK0), "given": (D, MASKD)}
ROW_SHAPES = ((2, 3, C), (ROWS, C), (1, 2, 3, C))    # the rotate forms take any leading dimensions
G6_TABLES = {"e1m2": 1, "fp_e1": 1, "e3m0": 2, "fp_e3": 2}
GF6_TABLES = {"e2m3": 3, "fp6_e2m3": 3, "e3m2": 4, "fp6_e3m2": 4}


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, tuple(("mask", tuple(a)) if isinstance(a, ctypes.Array) else a for a in args)))
            return 0
        return entry

    def take(self):
        calls, self.calls = self.calls, []
        return calls


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(rot, "_native", None)
    monkeypatch.setattr(rot, "require_gpu", lambda *a, **k: None)
    monkeypatch.setattr(rot, "stream_ptr", lambda device: 0)
    monkeypatch.setattr(rot, "device_guard", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(rot, "lib", lambda: r)
    return r


def named(calls, **tensors):
    """The recorded calls with every pointer replaced by the name of the tensor it is the address of (`tensors`: name -> tensor or
    None; a later name wins over an earlier one of the same address); the address of anything else becomes tmp0, tmp1, ... in the
    order of appearance."""
    names = {t.data_ptr(): n for n, t in tensors.items() if t is not None}
    def one(v):
        if isinstance(v, tuple):
            return v
        if isinstance(v, int) and not isinstance(v, bool) and v >= 1 << 16:
            return names.setdefault(v, f"tmp{sum(1 for n in names.values() if n.startswith('tmp'))}")
        return v
    out = []
    for name, args in calls:
        assert len(args) == len(_lib._SIGS[name][1]), (name, len(args))
        out.append((name, tuple(one(a) for a in args)))
    return out


class Tmp:
    """the expected name of a pointer: the tensor's own, or the next tmpN where the call had to copy it"""
    def __init__(self):
        self.n = 0

    def __call__(self, name, copied=True):
        if not copied:
            return name
        self.n += 1
        return f"tmp{self.n - 1}"


def rows_tensor(shape, dtype=f16, contiguous=True):
    if contiguous:
        return torch.zeros(*shape, dtype=dtype)
    t = torch.zeros(*shape[:-1], 2 * shape[-1], dtype=dtype)[..., ::2]
    assert not t.is_contiguous() and tuple(t.shape) == tuple(shape)
    return t


def smooth_of(kind):
    """(the argument, whether _smooth_ptr has to convert it)"""
    return {"none": (None, False), "f32": (torch.full((C,), 1.5), False), "scalar": (torch.tensor(2.0), True),
            "f16": (torch.full((C,), 1.5, dtype=f16), True)}[kind]


SMOOTHS = ("none", "f32", "scalar", "f16")


def mod_of(kind, dtype, bsz=2):
    """(scale, shift, whether _mod_rows has to copy them)"""
    if kind == "b1c":
        return torch.zeros(bsz, 1, C, dtype=dtype), torch.zeros(bsz, 1, C, dtype=dtype), False
    if kind == "bc":
        return torch.zeros(bsz, C, dtype=dtype), torch.zeros(bsz, C, dtype=dtype), False
    assert kind == "expanded"
    return torch.zeros(1, 1, C, dtype=dtype).expand(bsz, 1, C), torch.zeros(1, 1, C, dtype=dtype).expand(bsz, 1, C), True


MODS = (("b1c", f16), ("bc", f16), ("expanded", f16), ("b1c", f32), ("expanded", f32))


def returned(got, kind, xshape, km, extra=0):
    """`got` as a tuple, after checking count, shapes, dtypes and the zeroed padding of a k-major scale image.  kind: "values" (fp16 of
    x's shape, `extra` more of them with the intermediates), "fp4" / "g6" (per-group operands), "fp8" / "tok6" (per-token operands)"""
    rets = got if isinstance(got, tuple) else (got,)
    if kind == "values":
        want = [(tuple(xshape), f16)] * (1 + extra)
        assert isinstance(got, tuple) == (extra > 0)
    else:
        seg = {"fp4": 64, "g6": 96, "fp8": 128, "tok6": 96}[kind]
        codes = ((G, ROWS, seg) if km else (ROWS, G * seg), u8)
        if kind in ("fp8", "tok6"):
            scales = ((ROWS,), f16)
        else:
            scales = ((G, PAD), f32) if km else ((ROWS, G), f16)
        want = [codes, scales]
        assert isinstance(got, tuple)
    assert [(tuple(t.shape), t.dtype) for t in rets] == want
    assert all(t.is_contiguous() for t in rets)
    if km and kind in ("fp4", "g6"):
        assert not bool(rets[1][:, ROWS:].any()), "the padding columns of the scale image must be zero on return"
    return rets


def ret_names(rets, first=0):
    return {f"ret{first + i}": t for i, t in enumerate(rets)}


# ---- the plain rotate forms: x [..., C] ---------------------------------------------------------------------------------------------
# (function, {table: id} or None when it takes none, kind, entry point of a layout, what follows the mask: (table id, kmajor) -> tuple)
ROTATE_CODES = (
    ("rotate_quant_mx", None, "fp4", lambda km: "fpq_rotate_quant_rows_codes_mx_km" if km else "fpq_rotate_quant_rows_codes_mx",
     lambda tid, km: ()),
    ("rotate_quant_g6", G6_TABLES, "g6", lambda km: "fpq_a6w4_rotate_quant_rows_codes", lambda tid, km: (tid, int(km))),
    ("rotate_quant_gf6", GF6_TABLES, "g6", lambda km: "fpq_gf6_rotate_quant_rows_codes", lambda tid, km: (tid, int(km))),
)


@pytest.mark.parametrize("contiguous", (True, False))
@pytest.mark.parametrize("dtype", (f16, f32))
@pytest.mark.parametrize("shape", ROW_SHAPES)
def test_rotate_quant(rec, shape, dtype, contiguous):
    for table in ("e2m1", "e3m0", "e2m3"):
        for sign, (d, mask) in SIGNS.items():
            for sk in SMOOTHS:
                for rotated in (False, True):
                    x = rows_tensor(shape, dtype, contiguous)
                    sm, converted = smooth_of(sk)
                    got = rot.rotate_quant(x, table, d, sm, return_rotated=rotated)
                    rets = returned(got, "values", shape, False, extra=int(rotated))
                    tmp = Tmp()
                    want = (tmp("x", not contiguous), "ret0", "ret1" if rotated else None, ROWS, C, F32 if dtype is f32 else F16,
                            None if sm is None else tmp("smooth", converted), ("mask", mask), TID[table], 0)
                    assert named(rec.take(), **ret_names(rets), x=x, smooth=sm) == [("fpq_rotate_quant_rows", want)]


@pytest.mark.parametrize("km", (False, True))
@pytest.mark.parametrize("contiguous", (True, False))
@pytest.mark.parametrize("dtype", (f16, f32))
@pytest.mark.parametrize("shape", ROW_SHAPES)
@pytest.mark.parametrize("fn, tables, kind, entry, tail", ROTATE_CODES, ids=[r[0] for r in ROTATE_CODES])
def test_rotate_quant_operands(rec, fn, tables, kind, entry, tail, shape, dtype, contiguous, km):
    for table, tid in (tables or {None: None}).items():
        for sign, (d, mask) in SIGNS.items():
            for sk in SMOOTHS:
                x = rows_tensor(shape, dtype, contiguous)
                sm, converted = smooth_of(sk)
                kw = {} if table is None else {"table": table}
                rets = returned(getattr(rot, fn)(x, d=d, smooth=sm, kmajor=km, **kw), kind, shape, km)
                tmp = Tmp()
                want = (tmp("x", not contiguous), "ret0", "ret1", ROWS, C, F32 if dtype is f32 else F16,
                        None if sm is None else tmp("smooth", converted), ("mask", mask), *tail(tid, km), 0)
                assert named(rec.take(), **ret_names(rets), x=x, smooth=sm) == [(entry(km), want)]


def test_rotate_defaults(rec):
    """the default tables: e2m1, e3m0 (g6), e2m3 (gf6); row-major; no intermediates"""
    x = rows_tensor((ROWS, C))
    for fn, entry, tail in ((rot.rotate_quant, "fpq_rotate_quant_rows", (0,)), (rot.rotate_quant_g6, "fpq_a6w4_rotate_quant_rows_codes", (2, 0)),
                            (rot.rotate_quant_gf6, "fpq_gf6_rotate_quant_rows_codes", (3, 0)), (rot.rotate_quant_mx, "fpq_rotate_quant_rows_codes_mx", ())):
        fn(x)
        (name, args), = rec.take()
        assert name == entry and args[-1 - len(tail) - 1:] == (("mask", MASK0), *tail, 0)


# ---- the adaLN forms: x [B, L, C] with modulation rows -----------------------------------------------------------------------------
# (function, keyword arguments, table id or None, kind, entry point of a layout or None where the form has no k-major layout,
#  number of NULLs after `out`, what follows the mask)
def _km(name):
    return lambda km: name + "_km" if km else name


def _flag(name):
    return lambda km: name


ADALN = (
    ("adaln_rotate_quant_mx", {}, None, "fp4", _km("fpq_adaln_rotate_quant_rows_codes_mx"), lambda tid, km: ()),
    *[("adaln_rotate_quant_g6", {"table": t}, i, "g6", _flag("fpq_a6w4_adaln_rotate_quant_rows_codes"), lambda tid, km: (tid, int(km)))
      for t, i in G6_TABLES.items()],
    *[("adaln_rotate_quant_gf6", {"table": t}, i, "g6", _flag("fpq_gf6_adaln_rotate_quant_rows_codes"), lambda tid, km: (tid, int(km)))
      for t, i in GF6_TABLES.items()],
    ("adaln_rotate_quant_token", {"emit": "fp8", "table": "e2m3"}, 3, "fp8", None, lambda tid, km: (tid,)),
    ("adaln_rotate_quant_token", {"emit": "fp8", "table": "e3m2"}, 4, "fp8", None, lambda tid, km: (tid,)),
    ("adaln_rotate_quant_token", {"emit": "fp6", "table": "e2m3"}, 3, "tok6", _km("fpq_adaln_rotate_quant_token_rows_codes_fp6"),
     lambda tid, km: (tid,)),
    ("adaln_rotate_quant_token", {"emit": "bf6", "table": "e3m2"}, 4, "tok6", _flag("fpq_adaln_rotate_quant_token_rows_codes_f6"),
     lambda tid, km: (tid, int(km))),
)
ADALN_IDS = ["-".join([r[0], *r[1].values()]) for r in ADALN]


def adaln_case(rec, fn, kw, entry, kind, km, outs, tail, dtype, contiguous, sign, sk, mk, mdt, extra=0, eps=None):
    x = rows_tensor((2, 3, C), dtype, contiguous)
    d, mask = SIGNS[sign]
    sm, converted = smooth_of(sk)
    sc, sh, copied = mod_of(mk, mdt)
    kw = dict(kw, d=d, smooth=sm, **({} if eps is None else {"eps": eps}))
    rets = returned(getattr(rot, fn)(x, sc, sh, **kw), kind, (2, 3, C), km, extra)
    tmp = Tmp()
    want = (tmp("x", not contiguous), *outs, ROWS, C, F32 if dtype is f32 else F16, tmp("scale", copied), tmp("shift", copied),
            F32 if mdt is f32 else F16, 3, 1e-6 if eps is None else eps, None if sm is None else tmp("smooth", converted), ("mask", mask),
            *tail, 0)
    assert named(rec.take(), **ret_names(rets), x=x, scale=sc, shift=sh, smooth=sm) == [(entry, want)]


@pytest.mark.parametrize("contiguous", (True, False))
@pytest.mark.parametrize("dtype", (f16, f32))
@pytest.mark.parametrize("fn, kw, tid, kind, entry, tail", ADALN, ids=ADALN_IDS)
def test_adaln_operands(rec, fn, kw, tid, kind, entry, tail, dtype, contiguous):
    for km in (False, True) if entry is not None else (False,):
        name = "fpq_adaln_rotate_quant_token_rows_codes_fp8" if entry is None else entry(km)
        for sign in SIGNS:
            for sk in SMOOTHS:
                for mk, mdt in MODS:
                    adaln_case(rec, fn, dict(kw, kmajor=km), name, kind, km, ("ret0", "ret1"), tail(tid, km), dtype, contiguous, sign, sk, mk, mdt)
    adaln_case(rec, fn, kw, "fpq_adaln_rotate_quant_token_rows_codes_fp8" if entry is None else entry(False), kind, False, ("ret0", "ret1"),
               tail(tid, False), dtype, contiguous, "default", "none", "b1c", f16, eps=1e-5)


@pytest.mark.parametrize("contiguous", (True, False))
@pytest.mark.parametrize("dtype", (f16, f32))
def test_adaln_values(rec, dtype, contiguous):
    """adaln_rotate_quant (with and without its intermediates) and the per-token form's values"""
    for sign in SIGNS:
        for sk in SMOOTHS:
            for mk, mdt in MODS:
                for table in ("e2m1", "e1m2", "e2m3"):
                    adaln_case(rec, "adaln_rotate_quant", {"table": table}, "fpq_adaln_rotate_quant_rows", "values", False,
                               ("ret0", None, None), (TID[table],), dtype, contiguous, sign, sk, mk, mdt)
                    adaln_case(rec, "adaln_rotate_quant", {"table": table, "return_intermediates": True}, "fpq_adaln_rotate_quant_rows",
                               "values", False, ("ret0", "ret1", "ret2"), (TID[table],), dtype, contiguous, sign, sk, mk, mdt, extra=2)
                for table in ("e2m3", "e3m2"):
                    adaln_case(rec, "adaln_rotate_quant_token", {"table": table}, "fpq_adaln_rotate_quant_token_rows", "values", False,
                               ("ret0", None, None, None), (TID[table],), dtype, contiguous, sign, sk, mk, mdt)
    adaln_case(rec, "adaln_rotate_quant", {}, "fpq_adaln_rotate_quant_rows", "values", False, ("ret0", None, None), (0,), dtype, contiguous,
               "default", "none", "b1c", f16, eps=1e-5)                    # the default table: e2m1
    adaln_case(rec, "adaln_rotate_quant_token", {}, "fpq_adaln_rotate_quant_token_rows", "values", False, ("ret0", None, None, None), (3,),
               dtype, contiguous, "default", "none", "b1c", f16, eps=1e-5)   # e2m3, emit="values"
    adaln_case(rec, "adaln_rotate_quant_g6", {}, "fpq_a6w4_adaln_rotate_quant_rows_codes", "g6", False, ("ret0", "ret1"), (2, 0), dtype, contiguous,
               "default", "none", "b1c", f16)                             # e3m0, row-major
    adaln_case(rec, "adaln_rotate_quant_gf6", {}, "fpq_gf6_adaln_rotate_quant_rows_codes", "g6", False, ("ret0", "ret1"), (3, 0), dtype, contiguous,
               "default", "none", "b1c", f16)                             # e2m3, row-major


# ---- the forms with the gated residual in front ------------------------------------------------------------------------------------
# (function, keyword arguments, kind, entry point, NULLs after `out`, what follows the mask: kmajor -> tuple, k-major layouts)
RESID = (
    ("resid_adaln_rotate_quant", {"table": "e2m1"}, "values", "fpq_resid_adaln_rotate_quant_rows", 2, lambda km: (0,), (False,)),
    ("resid_adaln_rotate_quant", {"table": "e3m0"}, "values", "fpq_resid_adaln_rotate_quant_rows", 2, lambda km: (2,), (False,)),
    ("resid_adaln_rotate_quant_mx", {}, "fp4", "fpq_resid_adaln_rotate_quant_rows_codes_mx", 0, lambda km: (int(km),), (False, True)),
    ("resid_adaln_rotate_quant_token", {"table": "e2m3"}, "values", "fpq_resid_adaln_rotate_quant_token_rows", 3, lambda km: (3,), (False,)),
    ("resid_adaln_rotate_quant_token", {"table": "e3m2"}, "values", "fpq_resid_adaln_rotate_quant_token_rows", 3, lambda km: (4,), (False,)),
    ("resid_adaln_rotate_quant_token", {"table": "e2m3", "emit": "fp6"}, "tok6", "fpq_resid_adaln_rotate_quant_token_rows_codes_f6", 0,
     lambda km: (3, int(km)), (False, True)),
    ("resid_adaln_rotate_quant_token", {"table": "e3m2", "emit": "fp6"}, "tok6", "fpq_resid_adaln_rotate_quant_token_rows_codes_f6", 0,
     lambda km: (4, int(km)), (False, True)),
)
RESID_IDS = ["-".join([r[0], *r[1].values()]) for r in RESID]


def resid_case(rec, fn, kw, entry, kind, km, nulls, tail, dtype, inplace, y_contig, r_contig, sign, sk, mk, mdt, intermediates=False):
    y = rows_tensor((2, 3, C), f16, y_contig)
    gate, _, gate_copied = mod_of("expanded" if mk == "expanded" else mk, f16)
    res = rows_tensor((2, 3, C), dtype, r_contig)
    d, mask = SIGNS[sign]
    sm, converted = smooth_of(sk)
    sc, sh, copied = mod_of(mk, mdt)
    kw = dict(kw, d=d, smooth=sm, inplace=inplace)
    if km:
        kw["kmajor"] = True
    if intermediates:
        kw["return_intermediates"] = True
    got = getattr(rot, fn)(y, gate, res, sc, sh, **kw)
    assert isinstance(got, tuple)
    x_new = got[0]
    assert x_new.dtype is dtype and tuple(x_new.shape) == (2, 3, C) and x_new.is_contiguous() and (x_new is res) == inplace
    rest = returned(got[1:] if len(got) > 2 else got[1], kind, (2, 3, C), km, extra=2 if intermediates else 0)
    tmp = Tmp()
    # y, gate, x_new, residual: in place x_new IS the residual; otherwise a fresh tensor beside (a contiguous copy of) the residual
    head = (tmp("y", not y_contig), tmp("gate", gate_copied), "residual" if inplace else "ret0", tmp("residual", not r_contig))
    outs = ("ret1", "ret2", "ret3") if intermediates else ("ret1", *[None] * nulls) if kind == "values" else ("ret1", "ret2")
    want = (*head, *outs, ROWS, C, F32 if dtype is f32 else F16, tmp("scale", copied), tmp("shift", copied), F32 if mdt is f32 else F16, 3, 1e-6,
            None if sm is None else tmp("smooth", converted), ("mask", mask), *tail, 0)
    names = dict(ret_names((x_new,)), **ret_names(rest, 1), y=y, gate=gate, residual=res, scale=sc, shift=sh, smooth=sm)
    assert named(rec.take(), **names) == [(entry, want)]


@pytest.mark.parametrize("inplace", (False, True))
@pytest.mark.parametrize("dtype", (f16, f32))
@pytest.mark.parametrize("fn, kw, kind, entry, nulls, tail, layouts", RESID, ids=RESID_IDS)
def test_resid(rec, fn, kw, kind, entry, nulls, tail, layouts, dtype, inplace):
    for km in layouts:
        for y_contig in (True, False):
            for r_contig in (True, False) if not inplace else (True,):        # in place needs a contiguous residual
                for sign in SIGNS:
                    for sk in SMOOTHS:
                        for mk, mdt in MODS:
                            resid_case(rec, fn, kw, entry, kind, km, nulls, tail(km), dtype, inplace, y_contig, r_contig, sign, sk, mk, mdt)
    if fn == "resid_adaln_rotate_quant":
        for y_contig in (True, False):
            resid_case(rec, fn, kw, entry, kind, False, nulls, tail(False), dtype, inplace, y_contig, True, "default", "f32", "b1c", f16,
                       intermediates=True)


def test_resid_defaults(rec):
    """the default tables (e2m1; e2m3 for the per-token form), emit="values", row-major, a fresh x_new; eps is passed on"""
    y, res = rows_tensor((2, 3, C)), rows_tensor((2, 3, C))
    gate, sc, sh = torch.zeros(2, 1, C, dtype=f16), torch.zeros(2, 1, C, dtype=f16), torch.zeros(2, 1, C, dtype=f16)
    for fn, entry, tail in ((rot.resid_adaln_rotate_quant, "fpq_resid_adaln_rotate_quant_rows", (0,)),
                            (rot.resid_adaln_rotate_quant_mx, "fpq_resid_adaln_rotate_quant_rows_codes_mx", (0,)),
                            (rot.resid_adaln_rotate_quant_token, "fpq_resid_adaln_rotate_quant_token_rows", (3,))):
        got = fn(y, gate, res, sc, sh, eps=1e-5)
        assert got[0] is not res
        (name, args), = rec.take()
        assert name == entry and args[-1 - len(tail) - 1:] == (("mask", MASK0), *tail, 0) and 1e-5 in args and 1e-6 not in args


# ---- refusals: the present texts, the function's own name in front, in the order a call with two faults reports them --------------
def refused(rec, message, fn, *args, **kw):
    with pytest.raises(RuntimeError, match=message):
        fn(*args, **kw)
    assert not rec.calls, "a refused call reached the library"


BAD_SMOOTH = torch.ones(3)


def test_rotate_refusals(rec):
    x = rows_tensor((ROWS, C))
    refused(rec, r"^rotate_quant: x must be float16 or float32, got torch\.float64$", rot.rotate_quant, x.double())
    refused(rec, r"^rotate_quant: x must be float16 or float32, got torch\.bfloat16$", rot.rotate_quant, rows_tensor((ROWS, 100), torch.bfloat16))
    refused(rec, r"^rotate_quant: the last dimension must be a multiple of 128$", rot.rotate_quant, rows_tensor((ROWS, 100)))
    refused(rec, r"^rotate_quant: the last dimension must be a multiple of 128$", rot.rotate_quant, rows_tensor((ROWS, 100)), smooth=BAD_SMOOTH)
    refused(rec, r"^smooth must have one entry per channel$", rot.rotate_quant, x, smooth=BAD_SMOOTH)
    for name, bad_table, table_text in (("rotate_quant_mx", None, None),
                                        ("rotate_quant_g6", "e2m3", "the per-group 6-bit activation tables are 'e1m2' and 'e3m0', got 'e2m3'"),
                                        ("rotate_quant_gf6", "e3m0", "the per-group formats here are 'e2m3' and 'e3m2', got 'e3m0'")):
        fn = getattr(rot, name)
        shape_text = f"^{name}: x must be float16/float32 with a last dimension that is a multiple of 128$"
        refused(rec, shape_text, fn, x.double())
        refused(rec, shape_text, fn, rows_tensor((ROWS, 100)))
        refused(rec, r"^smooth must have one entry per channel$", fn, x, smooth=BAD_SMOOTH)
        if bad_table is not None:
            refused(rec, f"^{name}: {table_text}$", fn, x, bad_table)
            refused(rec, f"^{name}: {table_text[:-6]}None$", fn, x, None)
            refused(rec, shape_text, fn, x.double(), bad_table)                        # x before the table
            refused(rec, f"^{name}: {table_text}$", fn, x, bad_table, smooth=BAD_SMOOTH)   # the table before smooth


ADALN_FNS = (("adaln_rotate_quant", 4096, None, None), ("adaln_rotate_quant_mx", 4096, None, None),
             ("adaln_rotate_quant_g6", 2560, "e2m3", "the per-group 6-bit activation tables are 'e1m2' and 'e3m0', got 'e2m3'"),
             ("adaln_rotate_quant_gf6", 2560, "e1m2", "the per-group formats here are 'e2m3' and 'e3m2', got 'e1m2'"),
             ("adaln_rotate_quant_token", 2560, None, None))


@pytest.mark.parametrize("name, cap, bad_table, table_text", ADALN_FNS, ids=[r[0] for r in ADALN_FNS])
def test_adaln_refusals(rec, name, cap, bad_table, table_text):
    fn = getattr(rot, name)
    x = rows_tensor((2, 3, C))
    sc, sh, _ = mod_of("b1c", f16)
    dim, width, mods = rf"^{name}: x must be \[B, L, C\]$", f"^{name}: C must be a multiple of 128 and at most {cap}$", \
        f"^{name}: scale and shift must both be float16 or both float32$"
    wide = lambda c: (rows_tensor((1, 2, c)), torch.zeros(1, 1, c, dtype=f16), torch.zeros(1, 1, c, dtype=f16))
    refused(rec, dim, fn, x.view(ROWS, C), sc, sh)
    refused(rec, dim, fn, rows_tensor((ROWS, 100)), sc, sh.float())            # the rank before the width and the modulation's dtype
    refused(rec, width, fn, *wide(192))
    refused(rec, width, fn, *wide(cap + 128))
    refused(rec, width, fn, rows_tensor((1, 2, 192)), sc, sh.float())           # the width before the modulation's dtype
    refused(rec, mods, fn, x, sc, sh.float())
    refused(rec, mods, fn, x, sc.double(), sh.double())
    refused(rec, mods, fn, x, sc[:1], sh[:1].float())                           # the dtype before the shape
    refused(rec, r"shape '\[2, 256\]' is invalid for input of size 256", fn, x, sc[:1], sh[:1])   # torch's own, from the reshape to [B, C]
    refused(rec, r"^smooth must have one entry per channel$", fn, x, sc, sh, smooth=BAD_SMOOTH)
    if bad_table is not None:
        refused(rec, f"^{name}: {table_text}$", fn, x, sc, sh, bad_table)
        refused(rec, mods, fn, x, sc, sh.float(), bad_table)                    # the modulation's dtype before the table
        refused(rec, f"^{name}: {table_text}$", fn, x, sc[:1], sh[:1], bad_table)   # the table before the modulation's shape
        refused(rec, f"^{name}: {table_text}$", fn, x, sc, sh, bad_table, smooth=BAD_SMOOTH)


def test_adaln_token_refusals(rec):
    name, fn = "adaln_rotate_quant_token", rot.adaln_rotate_quant_token
    x = rows_tensor((2, 3, C))
    sc, sh, _ = mod_of("b1c", f16)
    unknown, fp6, bf6 = f"^{name}: unknown emit 'fp4'$", f"^{name}: emit='fp6' is the E2M3 operand format$", f"^{name}: emit='bf6' is the E3M2 operand format$"
    layout = rf"^{name}: kmajor is a layout of the FP6 operand codes \(emit='fp6' / 'bf6'\)$"
    refused(rec, unknown, fn, x, sc, sh, emit="fp4")
    refused(rec, unknown, fn, x, sc, sh, emit="fp4", kmajor=True)
    refused(rec, f"^{name}: scale and shift must both", fn, x, sc, sh.float(), emit="fp4")      # the shared checks before emit
    refused(rec, r"shape '\[2, 256\]' is invalid", fn, x, sc[:1], sh[:1], emit="fp4")
    refused(rec, fp6, fn, x, sc, sh, "e3m2", emit="fp6")
    refused(rec, fp6, fn, x, sc, sh, "fp6_e2m3", emit="fp6")                                    # one spelling only
    refused(rec, fp6, fn, x, sc, sh, "bogus", emit="fp6")
    refused(rec, bf6, fn, x, sc, sh, "e2m3", emit="bf6")
    refused(rec, bf6, fn, x, sc, sh, emit="bf6")                                                # the default table is e2m3
    refused(rec, layout, fn, x, sc, sh, kmajor=True)
    refused(rec, layout, fn, x, sc, sh, emit="fp8", kmajor=True)
    refused(rec, layout, fn, x, sc, sh, kmajor=True, smooth=BAD_SMOOTH)
    refused(rec, fp6, fn, x, sc, sh, "e3m2", emit="fp6", smooth=BAD_SMOOTH)


RESID_FNS = ("resid_adaln_rotate_quant", "resid_adaln_rotate_quant_mx", "resid_adaln_rotate_quant_token")


@pytest.mark.parametrize("name", RESID_FNS)
def test_resid_refusals(rec, name):
    """_resid_args' chain, each fault alone and with the next one of the chain beside it"""
    fn = getattr(rot, name)
    def base(c=C, b=2):
        return dict(y=rows_tensor((b, 3, c)), gate=torch.zeros(b, 1, c, dtype=f16), residual=rows_tensor((b, 3, c)),
                    scale=torch.zeros(b, 1, c, dtype=f16), shift=torch.zeros(b, 1, c, dtype=f16))
    def call(a, **kw):
        return lambda: fn(a["y"], a["gate"], a["residual"], a["scale"], a["shift"], **kw)
    def check(message, a, **kw):
        with pytest.raises(RuntimeError, match=message):
            call(a, **kw)()
        assert not rec.calls, "a refused call reached the library"
    a = base()
    check(rf"^{name}: residual must be \[B, L, C\]$", dict(a, residual=a["residual"].view(ROWS, C).double()))
    check(rf"^{name}: residual must be float16 or float32, got torch\.float64$", dict(base(192), residual=rows_tensor((2, 3, 192), torch.float64)))
    check(f"^{name}: C must be a multiple of 128 and at most 2560$", dict(base(192), y=rows_tensor((2, 3, 192), f32)))
    check(f"^{name}: C must be a multiple of 128 and at most 2560$", base(2688, 1))
    check(rf"^{name}: y and gate must be float16, got torch\.float32 and torch\.float16$", dict(a, y=rows_tensor((2, 2, C), f32)))
    check(rf"^{name}: y and gate must be float16, got torch\.float16 and torch\.float32$", dict(a, gate=a["gate"].float()))
    check(rf"^{name}: y \(2, 2, 256\) must have the shape of residual \(2, 3, 256\)$", dict(a, y=rows_tensor((2, 2, C)), gate=a["gate"][:1]))
    check(rf"^{name}: gate \(1, 1, 256\) must be \[B, 1, C\] \(or \[B, C\]\) for residual \(2, 3, 256\)$",
          dict(a, gate=a["gate"][:1], shift=a["shift"].float()))
    check(rf"^{name}: gate \(2, 3, 256\) must be", dict(a, gate=torch.zeros(2, 3, C, dtype=f16)))
    check(rf"^{name}: gate \(256, 2\) must be", dict(a, gate=torch.zeros(C, 2, dtype=f16)))
    check(f"^{name}: scale and shift must both be float16 or both float32$", dict(a, scale=a["scale"][:1], shift=a["shift"][:1].float()))
    check(f"^{name}: scale and shift must both be float16 or both float32$", dict(a, scale=a["scale"].double(), shift=a["shift"].double()))
    nc = a["residual"].transpose(0, 1).contiguous().transpose(0, 1)
    check(rf"^{name}: scale and shift must be \[B, 1, C\] \(or \[B, C\]\) for residual \(2, 3, 256\)$",
          dict(a, scale=a["scale"][:1], shift=a["shift"][:1], residual=nc), inplace=True)
    check(f"^{name}: inplace=True needs a contiguous residual$", dict(a, residual=nc), inplace=True)
    check(f"^{name}: inplace=True writes x_new over residual, which must not overlap y$", dict(a, residual=a["y"]), inplace=True)
    flat = torch.zeros(4 * 3 * C, dtype=f16)
    one = base(b=1)
    check(f"^{name}: inplace=True writes x_new over residual, which must not overlap y$",
          dict(one, y=flat[: 3 * C].view(1, 3, C), residual=flat[C: 4 * C].view(1, 3, C)), inplace=True)
    check(f"^{name}: inplace=True writes x_new over residual, which must not overlap y$", dict(a, residual=a["y"]), inplace=True, smooth=BAD_SMOOTH)
    check("^smooth must have one entry per channel$", a, smooth=BAD_SMOOTH)
    call(dict(a, residual=a["y"]))()                      # not in place the same tensor may be both
    call(dict(one, y=flat[: 6 * C].view(1, 3, 2 * C)[..., ::2], residual=flat[: 3 * C].view(1, 3, C)), inplace=True)()   # a copy of y cannot overlap
    assert len(rec.take()) == 2
    if name == "resid_adaln_rotate_quant_token":
        check(f"^{name}: emit must be 'values' or 'fp6', got 'fp8'$", a, emit="fp8", kmajor=True)
        check(f"^{name}: emit must be 'values' or 'fp6', got 'bf6'$", a, emit="bf6", table="e2m1")
        check(f"^{name}: y and gate must be float16", dict(a, gate=a["gate"].float()), emit="fp8")    # the shared checks before emit
        check(f"^{name}: emit='fp6' writes E2M3 or E3M2 codes, got table 'e2m1'$", a, emit="fp6", table="e2m1", kmajor=True)
        check(f"^{name}: emit='fp6' writes E2M3 or E3M2 codes, got table 'fp6_e2m3'$", a, emit="fp6", table="fp6_e2m3")
        check(rf"^{name}: kmajor is a layout of the 6-bit operand codes \(emit='fp6'\)$", a, kmajor=True, smooth=BAD_SMOOTH)
