"""CPU: the host side of the fused format search - the row weights, the winner rule, the refusals of search_layer(fused=True),
and the C ABI's declaration of fpq_sqerr_rows_weighted with the argument checks that need no GPU."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, DTYPE, SHAPE = 0, -1, -2, -3
PTR = 0x7000_0000_1000


def test_sample_row_weights():
    from fpqvar_amd import format_search as fs
    rows, outs = [2, 8, 18, 1, 512], 384
    got = fs.sample_row_weights(rows, outs, "cpu")
    assert got.dtype == torch.float32 and got.shape == (sum(rows),) and got.device.type == "cpu"
    want64 = torch.cat([torch.full((r,), 1.0 / (r * outs), dtype=torch.float64) for r in rows])
    assert torch.equal(got, want64.float()), "the float64 weights rounded to fp32"
    # the expression search_layer(batched=True) builds inline, bit for bit
    inline = torch.repeat_interleave(torch.tensor([1.0 / (r * outs) for r in rows], dtype=torch.float32), torch.tensor(rows))
    assert torch.equal(got.view(torch.int32), inline.view(torch.int32))
    # its dot with per-row sums is sum_j mean_j
    g = torch.Generator().manual_seed(0)
    outs = 6
    samples = [torch.rand(r, outs, generator=g, dtype=torch.float64) for r in (2, 5, 1)]
    row_sums = torch.cat([s.sum(dim=1) for s in samples])
    w = fs.sample_row_weights([2, 5, 1], outs, "cpu").double()
    assert abs(float(torch.dot(row_sums, w)) - sum(float(s.mean()) for s in samples)) < 1e-6


def test_pick_winner_is_search_layers_rule():
    from fpqvar_amd import format_search as fs
    f3, f2 = fs.FP4_FORMATS, fs.FP6_FORMATS

    def old_rule(table, formats):
        losses = {(wf, af): float(table[i][j]) for i, wf in enumerate(formats) for j, af in enumerate(formats)}
        return min(losses, key=lambda k: (losses[k], formats.index(k[0]), formats.index(k[1])))

    tables = [
        (f3, [[3.0, 2.0, 5.0], [4.0, 1.0, 6.0], [7.0, 8.0, 9.0]]),
        (f3, [[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]),          # all tied: (0, 0)
        (f3, [[2.0, 1.0, 1.0], [1.0, 2.0, 2.0], [1.0, 1.0, 3.0]]),          # tied across rows: the smaller weight index
        (f3, [[5.0, 5.0, 4.0], [4.0, 9.0, 9.0], [4.0, 4.0, 4.0]]),
        (f2, [[0.5, 0.25], [0.25, 0.5]]),
        (f2, [[float("inf"), 2.0], [3.0, float("inf")]]),
    ]
    for formats, t in tables:
        assert fs.pick_winner(t, formats) == old_rule(t, formats), t
        assert fs.pick_winner(torch.tensor(t, dtype=torch.float32), formats) == old_rule(t, formats), t
    assert fs.pick_winner(tables[1][1], f3) == ("fp_e1", "fp_e1")
    assert fs.pick_winner(tables[2][1], f3) == ("fp_e1", "fp_e2")
    assert fs.pick_winner(tables[4][1], f2) == ("fp6_e2m3", "fp6_e3m2")
    # search_layer itself (the sample loop, an injected quantizer that runs on the CPU) goes through it: same winner as the rule
    q = lambda fmt: (lambda t: (t * 4).round() / 4) if fmt == "fp6_e2m3" else (lambda t: (t * 2).round() / 2)
    g = torch.Generator().manual_seed(1)
    xs, w = [torch.randn(3, 16, generator=g) for _ in range(4)], torch.randn(8, 16, generator=g)
    wf, af, losses = fs.search_layer(xs, w, f2, quant=q)
    assert (wf, af) == min(losses, key=lambda k: (losses[k], f2.index(k[0]), f2.index(k[1]))) == ("fp6_e2m3", "fp6_e2m3")


def test_fused_form_refuses_what_it_cannot_run():
    from fpqvar_amd import format_search as fs
    g = torch.Generator().manual_seed(2)
    xs, w = [torch.randn(2, 4, 256, generator=g).half() for _ in range(3)], torch.randn(384, 256, generator=g).half()
    with pytest.raises(RuntimeError, match="CUDA"):
        fs.search_layer(xs, w, fs.FP6_FORMATS, fused=True)
    with pytest.raises(RuntimeError, match="batched"):
        fs.search_layer(xs, w, fs.FP6_FORMATS, batched=False, fused=True)
    with pytest.raises(RuntimeError, match="batched"):
        fs.search_layer(xs, w, fs.FP6_FORMATS, quant=lambda f: (lambda t: t), fused=True)      # an injected quantizer: the loop
    with pytest.raises(RuntimeError, match="fused"):
        fs.search_layer(xs, w, fs.FP6_FORMATS, losses_out=torch.empty(2, 2))
    with pytest.raises(RuntimeError, match="CUDA"):
        fs.search_layers_fused([(xs, w)], fs.FP6_FORMATS)
    from fpqvar_amd import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.sqerr_rows_weighted(torch.zeros(4, 8).half(), torch.zeros(4, 8).half(), torch.ones(4))
    for name in ("sample_row_weights", "pick_winner", "search_layers_fused", "search_blocks_sharded_fused"):
        assert callable(getattr(fs, name)), name


def test_entry_point_is_declared_bound_and_versioned():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fpq.h")).read()
    assert int(re.search(r"#define FPQ_VERSION (\d+)", hdr).group(1)) == 136
    assert re.search(r"int fpq_sqerr_rows_weighted\(const void\* ref, const void\* y, const float\* row_weight, float\* out, void\* workspace,"
                     r"\s+int64_t rows, int64_t cols, int planes, int dtype, fpq_stream_t stream\);", hdr)
    assert "fpq_sqerr_rows_weighted" in _lib._SIGS and len(_lib._SIGS["fpq_sqerr_rows_weighted"][1]) == 10
    assert _lib.SQERR_WORKSPACE_BYTES == int(re.search(r"#define FPQ_SQERR_WORKSPACE_BYTES (\d+)", hdr).group(1))
    lib = _lib.lib()
    assert lib.fpq_version() == 136
    from fpqvar_amd import _native
    assert callable(_native.sqerr_rows_weighted)


def test_refusals_and_their_order():
    """Every call below is refused before anything is enqueued; the pointers are a fake, aligned address that is never read."""
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    f = _lib.lib().fpq_sqerr_rows_weighted

    def call(ref=PTR, y=PTR, w=PTR, out=PTR, ws=PTR, rows=4, cols=16, planes=2, dtype=0):
        return f(ref, y, w, out, ws, rows, cols, planes, dtype, None)

    for kw in (dict(ref=None), dict(y=None), dict(w=None), dict(out=None), dict(ws=None), dict(rows=-1), dict(cols=-8), dict(planes=0),
               dict(planes=5)):
        assert call(**kw) == ARG, kw
    assert call(dtype=2) == DTYPE and call(dtype=7) == DTYPE
    for kw in (dict(cols=0), dict(cols=12), dict(cols=12, dtype=0), dict(cols=6, dtype=1), dict(rows=2 ** 31)):
        assert call(**kw) == SHAPE, kw
    for kw in (dict(ref=PTR + 8), dict(y=PTR + 2), dict(w=PTR + 4), dict(out=PTR + 2)):
        assert call(**kw) == ARG, kw
    # the order: argument, dtype, shape, alignment
    assert call(planes=0, dtype=7, cols=12, y=PTR + 2) == ARG
    assert call(dtype=7, cols=12, y=PTR + 2) == DTYPE
    assert call(cols=12, y=PTR + 2) == SHAPE
    assert call(cols=12, dtype=1, y=PTR + 2) == ARG      # 12 fp32 columns are whole vectors: only the alignment is left to refuse
