"""tests/block_model.py on small parameters of its own (C = 512, 8 heads, hidden 2048, depth 2, 2 rows, steps of 1, 4 and 9
tokens; weights quantized with the oracle): the model is what tests/test_gpu_block_paths.py holds the three generation paths to, so
it has to be right on its own evidence - the weight-side / activation-side pairing compensates exactly, it is deterministic, its
cache quantizer is idempotent, and every wiring mutant it offers moves the block update somewhere."""
import functools

import pytest
import torch

from fpqvar_amd import rotation as rot
from oracle import fpq_oracle as orc
from tests import block_model as bm

C, H, HID, DEPTH, ROWS, STEPS = 512, 8, 2048, 2, 2, (1, 4, 9)
REGIMES = [(config, l2) for config in ("w4a4", "w6a6") for l2 in (False, True)]


@functools.lru_cache(maxsize=None)
def _raw():
    """raw fp32-valued weights, smoothing vectors, modulation, l2 parameters and inputs, drawn once (read-only)"""
    g = torch.Generator().manual_seed(5)
    w = {n: (torch.randn(o, i, generator=g) * 0.02).double() for n, (o, i) in
         dict(qkv=(3 * C, C), proj=(C, C), fc1=(HID, C), fc2=(C, HID)).items()}
    s = {n: (torch.rand(C, generator=g) + 0.5).double() for n in ("qkv", "fc1")}
    mods = [[(torch.randn(ROWS, 1, C, generator=g) * 0.2).half() for _ in range(6)] for _ in range(DEPTH)]
    scale_mul = []
    for _ in range(DEPTH):
        sm = torch.full((1, H, 1, 1), 4.0).log() + 0.3 * torch.randn(1, H, 1, 1, generator=g)
        sm[0, 0] = bm.MAX_SCALE_MUL + 0.5          # one head above the clamp
        scale_mul.append(sm)
    bias = [torch.cat((torch.randn(C, generator=g) * 0.1, torch.zeros(C), torch.randn(C, generator=g) * 0.1)) for _ in range(DEPTH)]
    xs = [torch.randn(ROWS, n, C, generator=g).half() for n in STEPS]
    return w, s, mods, scale_mul, bias, xs


def _prepared(w, s, Q):
    """the reference's offline weight side: W / s per input channel, then W . Q (mat_qkv and fc1)"""
    out = dict(w)
    out["qkv"] = rot.rotate_weight(rot.transform_weight(w["qkv"], s["qkv"]), Q)
    out["fc1"] = rot.rotate_weight(rot.transform_weight(w["fc1"], s["fc1"]), Q)
    return out


@functools.lru_cache(maxsize=None)
def _params(config, l2):
    w, s, mods, scale_mul, bias, _ = _raw()
    Q = orc.block_hadamard(C, 128, 42)
    wq = {n: bm.CONFIGS[config]["weight"](t.float()) for n, t in _prepared(w, s, Q).items()}
    return bm.BlockParams(C=C, H=H, config=config, w=wq, mods=mods, s_qkv=s["qkv"].float(), s_fc1=s["fc1"].float(), Q=Q.float(),
                          scale_mul=scale_mul if l2 else None, qkv_bias=bias if l2 else None)


@functools.lru_cache(maxsize=None)
def _base(config, l2):
    return bm.run(_params(config, l2), _raw()[5])


@pytest.mark.parametrize("l2", [False, True])
def test_compensation(l2):
    """No quantizer, no fp16 rounding, raw weights w: the block on (w / s) Q with the activation side smoothed and rotated equals
    the block on w with neither, to float64 round-off.  Q here is the block Hadamard matrix over the float64 square root: the
    reference divides by float32(sqrt(128)), which leaves Q Q^T = (1 - 3.4e-8) I, not round-off."""
    w, s, mods, scale_mul, bias, xs = _raw()
    Q = orc.block_hadamard(C, 128, 42) * (float(torch.tensor(128).sqrt()) / 128 ** 0.5)
    assert float((Q @ Q.T - torch.eye(C, dtype=torch.float64)).abs().max()) < 1e-15
    common = dict(C=C, H=H, config="w4a4", mods=mods, ideal=True, scale_mul=scale_mul if l2 else None, qkv_bias=bias if l2 else None)
    plain = bm.run(bm.BlockParams(w=w, **common), xs)
    paired = bm.run(bm.BlockParams(w=_prepared(w, s, Q), s_qkv=s["qkv"], s_fc1=s["fc1"], Q=Q, **common), xs)
    dev = bm.deviation(paired, plain, xs)
    print(f"compensation, attn_l2_norm={l2}: deviation {dev:.2e}")
    assert dev < 1e-12
    # and it is a check: either factor alone does not compensate
    for half in (dict(s_qkv=s["qkv"], s_fc1=s["fc1"]), dict(Q=Q)):
        assert bm.deviation(bm.run(bm.BlockParams(w=_prepared(w, s, Q), **half, **common), xs), plain, xs) > 0.1


@pytest.mark.parametrize("config,l2", REGIMES)
def test_deterministic(config, l2):
    again = bm.run(_params(config, l2), _raw()[5])
    for a, b in zip(again, _base(config, l2)):
        assert torch.equal(a, b)
        assert torch.isfinite(a).all() and torch.equal(a, a.half().double())          # fp16 values


@pytest.mark.parametrize("config,l2", REGIMES)
def test_cache_requantization_is_idempotent(config, l2):
    """The whole cache is re-quantized at every step (tr/basic_var.py:186-209): from the second time on that changes nothing.
    An fp16 cache (plain regime) is a fixed point after ONE pass (tests/test_kv_idempotence.py).  Under attn_l2_norm the cache is
    fp32 (here float64) and the pass rounds its result to fp16: the second pass derives its scale from the rounded maximum, s' =
    half(7.5 s) / 7.5, and may move entries by an fp16 ulp; from then on the maximum is 7.5 s' itself and nothing moves."""
    model = bm.BlockModel(_params(config, l2))
    for x in _raw()[5]:
        model.step(x)
    last = STEPS[-1]
    for K, V in model.caches:
        assert K.shape[1] == sum(STEPS)
        for t in (K, V):
            once = model.quantize_cache(t)
            assert not torch.equal(once[:, -last:], t[:, -last:])          # the last step's entries: quantized for the first time
            assert torch.equal(once[:, :STEPS[0]], t[:, :STEPS[0]])        # the first step's: twice before
            twice = model.quantize_cache(once)
            assert torch.equal(model.quantize_cache(twice), twice)
            if not l2:
                assert torch.equal(twice, once)


@functools.lru_cache(maxsize=None)
def _table():
    return {r: bm.mutant_table(_params(*r), _raw()[5], _base(*r)) for r in REGIMES}


def format_table(table, title):
    """table: (config, l2) -> {mutant: deviation}; the printed form that profiles/block_paths_vs_model.txt records"""
    regimes = list(table)
    lines = [title, f"{'':>3} {'mutant':<30}" + "".join(f"{c + ('+l2' if l2 else ''):>12}" for c, l2 in regimes)]
    for i, m in enumerate(bm.MUTANTS):
        lines.append(f"{i + 1:>3} {m:<30}" + "".join(f"{table[r][m]:>12.4f}" for r in regimes))
    return "\n".join(lines)


def test_mutant_table():
    """Every mutant's deviation from the unmutated model, per regime.  Each must move the update by a clearly non-zero amount in at
    least one regime: ten times what rounding the residual stream to fp16 does to the same measure (2^-11 ||y|| / ||y - x||)."""
    table = _table()
    print("\n" + format_table(table, f"mutant deviations, C = {C}, depth {DEPTH}, {ROWS} rows, steps of {STEPS} tokens"))
    xs = _raw()[5]
    for m in bm.MUTANTS:
        clear = []
        for r in REGIMES:
            y = torch.cat([t.reshape(-1) for t in _base(*r)])
            x = torch.cat([t.double().reshape(-1) for t in xs])
            clear.append(table[r][m] >= 10 * 2.0 ** -11 * float(y.norm() / (y - x).norm()))
        assert any(clear), f"{m}: {[table[r][m] for r in REGIMES]}"
    for r in REGIMES:          # the l2-only mutants do nothing in the plain regime
        if not r[1]:
            assert table[r]["bias_dropped"] == 0.0 and table[r]["clamp_dropped"] == 0.0
