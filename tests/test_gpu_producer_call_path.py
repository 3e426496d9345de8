"""GPU: the two routes of rotation.py's twelve producers - the compiled binding, and ctypes with `rot._native` taken away - end in the
same C entry point, so everything they return is equal bit for bit: every tensor in full, x_new and the padding of a k-major scale
image included.  No tolerance is involved.  Which route a call takes is told by whether the binding was entered at all (a counting
proxy in the place of `rot._native`), not by the binding's function names."""
import functools

import pytest
import torch

from fpqvar_amd import rotation as rot

pytestmark = pytest.mark.gpu

C = 256
SHAPES = ((2, 5, C), (7, 19, C))   # 10 rows: a ragged group of four in the image padding, two batches, two 128-groups; 133 rows: more than one 128-row tile, ragged
f16, f32 = torch.float16, torch.float32

# function -> [(keyword arguments, whether the form has a k-major layout)]: one table per family, and e3m2 for the 6-bit forms; every emit
PLAIN = {"rotate_quant": [({"table": "e2m1"}, False), ({"table": "e3m2"}, False)],
         "rotate_quant_mx": [({}, True)],
         "rotate_quant_g6": [({"table": "e3m0"}, True)],
         "rotate_quant_gf6": [({"table": "e2m3"}, True), ({"table": "e3m2"}, True)]}
ADALN = {"adaln_rotate_quant": [({"table": "e2m1"}, False), ({"table": "e3m2"}, False)],
         "adaln_rotate_quant_mx": [({}, True)],
         "adaln_rotate_quant_g6": [({"table": "e3m0"}, True)],
         "adaln_rotate_quant_gf6": [({"table": "e2m3"}, True), ({"table": "e3m2"}, True)],
         "adaln_rotate_quant_token": [({"table": "e2m3", "emit": "values"}, False), ({"table": "e3m2", "emit": "values"}, False),
                                      ({"table": "e2m3", "emit": "fp8"}, False), ({"table": "e2m3", "emit": "fp6"}, True),
                                      ({"table": "e3m2", "emit": "bf6"}, True)]}
RESID = {"resid_adaln_rotate_quant": [({"table": "e2m1"}, False), ({"table": "e3m2"}, False)],
         "resid_adaln_rotate_quant_mx": [({}, True)],
         "resid_adaln_rotate_quant_token": [({"table": "e2m3", "emit": "values"}, False), ({"table": "e2m3", "emit": "fp6"}, True),
                                            ({"table": "e3m2", "emit": "fp6"}, True)]}
FUNCTIONS = {**PLAIN, **ADALN, **RESID}
INTERMEDIATES = {"rotate_quant": "return_rotated", "adaln_rotate_quant": "return_intermediates", "resid_adaln_rotate_quant": "return_intermediates"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def tensors(dev, shape, row_dtype, mod_dtype):
    """seeded inputs of a shape, made once: (x / residual, scale, shift, y, gate, a float32 smooth whose values fp16 holds exactly)"""
    g = torch.Generator().manual_seed(sum(shape) + (row_dtype is f32) + 2 * (mod_dtype is f32))
    b = shape[0]
    x = torch.randn(*shape, generator=g).to(row_dtype).to(dev)
    sc = (torch.randn(b, 1, C, generator=g) * 0.3).to(mod_dtype).to(dev)
    sh = (torch.randn(b, 1, C, generator=g) * 0.3).to(mod_dtype).to(dev)
    y = torch.randn(*shape, generator=g).half().to(dev)
    gate = (torch.randn(b, 1, C, generator=g) * 0.5).half().to(dev)
    sm = (torch.rand(C, generator=g) + 0.5).half().float().to(dev)
    return x, sc, sh, y, gate, sm


def call(name, t, kw, x=None):
    """the producer on the inputs `t` (x: another tensor in the place of the rows); an in-place call gets a copy of the residual"""
    rows, sc, sh, y, gate, _ = t
    rows = rows if x is None else x
    fn = getattr(rot, name)
    if name in PLAIN:
        return fn(rows, **kw)
    if name in ADALN:
        return fn(rows, sc, sh, **kw)
    return fn(y, gate, rows.clone() if kw.get("inplace") else rows, sc, sh, **kw)


class Counting:
    """in the place of the compiled binding: counts the calls that enter it"""
    def __init__(self, native):
        self._native, self.entered = native, 0

    def __getattr__(self, name):
        attr = getattr(self._native, name)
        if not callable(attr):
            return attr
        def entry(*a, **k):
            self.entered += 1
            return attr(*a, **k)
        return entry


def routed(monkeypatch, fn, entered):
    """fn() as built, which must enter the binding `entered` times"""
    assert rot._native is not None, "the compiled binding is not built"
    with monkeypatch.context() as m:
        proxy = Counting(rot._native)
        m.setattr(rot, "_native", proxy)
        got = fn()
        assert proxy.entered == entered, f"the binding was entered {proxy.entered} times, not {entered}"
    return got


def through_ctypes(monkeypatch, fn):
    with monkeypatch.context() as m:
        m.setattr(rot, "_native", None)
        return fn()


def same(a, b, what):
    assert isinstance(a, tuple) == isinstance(b, tuple), what
    a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    assert len(a) == len(b), what
    for i, (p, q) in enumerate(zip(a, b)):
        assert p.dtype == q.dtype and p.shape == q.shape, f"{what}[{i}]: {p.dtype} {tuple(p.shape)} != {q.dtype} {tuple(q.shape)}"
        assert torch.equal(p.contiguous().view(torch.uint8), q.contiguous().view(torch.uint8)), f"{what}[{i}]: bytes differ"


def layouts(kw, km):
    return [dict(kw, kmajor=k) for k in (False, True)] if km else [kw]


@pytest.mark.parametrize("name", FUNCTIONS)
def test_both_routes_return_the_same_bits(dev, monkeypatch, name):
    cases = [(shape, rows, f16, with_smooth, kw) for shape in SHAPES for rows in (f16, f32) for with_smooth in (False, True)
             for variant, km in FUNCTIONS[name] for kw in layouts(variant, km)]
    if name not in PLAIN:   # fp32 modulation, once per function
        cases += [(SHAPES[0], f16, f32, True, kw) for kw in layouts(*FUNCTIONS[name][0])]
    for shape, rows, mod, with_smooth, kw in cases:
        t = tensors(dev, shape, rows, mod)
        for extra in ({"inplace": False}, {"inplace": True}) if name in RESID else ({},):
            what = f"{name} {shape} rows {rows} modulation {mod} {dict(kw, **extra)} smooth {with_smooth}"
            args = dict(kw, smooth=t[5] if with_smooth else None, **extra)
            same(routed(monkeypatch, lambda: call(name, t, args), 1), through_ctypes(monkeypatch, lambda: call(name, t, args)), what)


@pytest.mark.parametrize("name", FUNCTIONS)
def test_what_the_binding_does_not_take(dev, monkeypatch, name):
    """a sign vector of the caller's, non-contiguous rows, the intermediates and a smooth vector that needs conversion go through ctypes -
    and, being the usual call's arguments in another form, return the usual call's bits"""
    t = tensors(dev, SHAPES[0], f16, f16)
    variant, km = FUNCTIONS[name][0]
    kw = dict(variant, smooth=t[5], **({"kmajor": True} if km else {}))
    usual = routed(monkeypatch, lambda: call(name, t, kw), 1)
    same(routed(monkeypatch, lambda: call(name, t, dict(kw, d=rot.sign_vector(128, 42))), 0), usual, name + ": d given")
    wide = torch.zeros(*SHAPES[0][:-1], 2 * C, dtype=f16, device=dev)
    wide[..., ::2] = t[0]
    assert not wide[..., ::2].is_contiguous()
    same(routed(monkeypatch, lambda: call(name, t, kw, x=wide[..., ::2]), 0), usual, name + ": non-contiguous rows")
    same(routed(monkeypatch, lambda: call(name, t, dict(kw, smooth=t[5].half())), 0), usual, name + ": an fp16 smooth vector")
    if name in INTERMEDIATES:
        got = routed(monkeypatch, lambda: call(name, t, dict(kw, **{INTERMEDIATES[name]: True})), 0)
        n = len(usual) if isinstance(usual, tuple) else 1
        assert isinstance(got, tuple) and len(got) == n + (1 if name == "rotate_quant" else 2)
        same(got[:n] if n > 1 else got[0], usual, name + ": with the intermediates")
    if name in RESID:   # a non-contiguous y as well
        y = torch.zeros(*SHAPES[0][:-1], 2 * C, dtype=f16, device=dev)
        y[..., ::2] = t[3]
        same(routed(monkeypatch, lambda: call(name, (t[0], t[1], t[2], y[..., ::2], t[4], t[5]), kw), 0), usual, name + ": non-contiguous y")
