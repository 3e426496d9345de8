"""fpq_attention_blhc (ops.attention_blhc) against a float64 reference with the per-element bound of
tests/attention_model.py, over the input families, a pairwise sweep of the shapes where the kernel's tiling changes, every
step of both models, and the calls the model itself makes.  Also: the layouts the model hands over (views of the qkv output
and of the KV-cache slab) give the same bits as contiguous copies, nothing at or past lkv and nothing outside the views is
read, and the results are bitwise invariant under batch, head and query-row permutations."""
import pytest
import torch

from tests import attention_model as am

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def _as_model_layout(q, k, v, dev):
    """q as a view of a [B, L, 3, H, 64] qkv output, k / v as views of a [2, B, max_len, H, 64] slab with max_len > Lkv; the
    qkv output's k / v slots and the slab's tail are NaN."""
    B, Lq, H, _ = q.shape
    Lkv = k.shape[1]
    qkv = torch.full((B, Lq, 3, H, 64), float("nan"), dtype=torch.float16, device=dev)
    qkv[:, :, 0] = q.to(dev)
    slab = torch.full((2, B, Lkv + 9, H, 64), float("nan"), dtype=torch.float16, device=dev)
    slab[0, :, :Lkv] = k.to(dev)
    slab[1, :, :Lkv] = v.to(dev)
    return qkv[:, :, 0], slab[0, :, :Lkv], slab[1, :, :Lkv]


def _check(worst, bad, family, q, k, v, scale, dev):
    """Views (NaN around them) and contiguous copies must give the same bits; the ratio to the bound goes to `worst`
    (per family) and, above 1, to `bad`."""
    qv, kv, vv = _as_model_layout(q, k, v, dev)
    out = _attn(qv, kv, vv, scale)
    out_c = _attn(qv.contiguous(), kv.contiguous(), vv.contiguous(), scale)
    assert torch.equal(out.view(torch.int16), out_c.view(torch.int16)), (family, tuple(q.shape), tuple(k.shape))
    r = am.reference(qv, kv, vv, scale)
    rat = _note(worst, family, out, r)
    if not rat <= 1.0:
        bad.append((family, tuple(q.shape), tuple(k.shape), rat))


def _attn(q, k, v, scale):
    from fpqvar_amd import ops
    return ops.attention_blhc(q, k, v, scale)


def _note(worst, name, out, r):
    """Keep the largest err / bound of `name`: over all elements and over those with |ref| >= 2^-14 (below, an output is
    a few steps of the 2^-24 subnormal grid and the bound is the worst case of two roundings).  -> the ratio."""
    rat, rat_n = am.ratio(out, r), am.ratio(out, r, normal_only=True)
    all_, normal = worst.get(name, (0.0, 0.0))
    worst[name] = (max(all_, rat), max(normal, rat_n))
    return rat


def _report(title, worst, bad):
    print(f"\n{title}: max err / bound, all elements / |ref| >= 2^-14")
    for name, (rat, rat_n) in sorted(worst.items(), key=lambda kv: -kv[1][1]):
        print(f"  {name:30s} {rat:.3f}  {rat_n:.3f}")
    assert not bad, f"{len(bad)} outside the bound, first {bad[:8]}"


def test_attention_families_over_the_shape_sweep(dev):
    """Every family over the pairwise (Lkv, Lq, B*H) sweep (odd and even tile counts, partial last tiles, the query-tile
    and wavefront edges, 8 (batch, head) pairs per group), every family once more at a four-tile Lkv with a partial tile."""
    worst, bad = {}, []
    for family, B, H, Lq, Lkv in am.shape_sweep():
        _check(worst, bad, family, *am.make_case(family, B, H, Lq, Lkv), dev)
    for i, family in enumerate(am.FAMILIES):
        _check(worst, bad, family, *am.make_case(family, 2, 5, 97, 225, seed=i + 1), dev)
    _report("families", worst, bad)


@pytest.mark.parametrize("model", ("d30-256", "d36-512"))
def test_attention_every_model_step(dev, model):
    """Lq = pn^2, Lkv = the running sum, H = the model's heads, at 2 rows in the l2-norm and the plain regime; the last step
    again at the model's full batch (100 / 20 rows)."""
    from fpqvar_amd.var_block import MODELS
    heads, patch_nums, rows = MODELS[model]
    worst, bad = {}, []
    calls = am.model_calls(patch_nums, heads)
    for family in ("l2norm", "plain", "l2norm_indicator"):
        for i, (H, Lq, Lkv) in enumerate(calls):
            _check(worst, bad, f"{model} {family}", *am.make_case(family, 2, H, Lq, Lkv, seed=i), dev)
    H, Lq, Lkv = calls[-1]
    _check(worst, bad, f"{model} l2norm B={rows}", *am.make_case("l2norm", rows, H, Lq, Lkv), dev)
    _report(model, worst, bad)


def test_attention_bitwise_invariances(dev):
    """One workgroup per (batch, head, 128 query rows) and a query row per lane: permuting batch entries, heads (the same
    permutation on q, k and v) or query rows permutes the output bit for bit, and a repeated call gives the same bits."""
    B, H, Lq, Lkv = 3, 5, 161, 193
    q, k, v, scale = (t.to(dev) if torch.is_tensor(t) else t for t in am.make_case("l2norm", B, H, Lq, Lkv))
    out = _attn(q, k, v, scale)
    assert torch.equal(_attn(q, k, v, scale).view(torch.int16), out.view(torch.int16))
    g = torch.Generator().manual_seed(5)
    pb, ph, pq = (torch.randperm(n, generator=g).to(dev) for n in (B, H, Lq))
    assert torch.equal(_attn(q[pb], k[pb], v[pb], scale).view(torch.int16), out[pb].view(torch.int16))
    assert torch.equal(_attn(q[:, :, ph], k[:, :, ph], v[:, :, ph], scale).view(torch.int16), out[:, :, ph].view(torch.int16))
    assert torch.equal(_attn(q[:, pq], k, v, scale).view(torch.int16), out[:, pq].view(torch.int16))


@pytest.mark.parametrize("model,path,l2", [("d36-512", "Q", True), ("d36-512", "F", True), ("d30-256", "Q", False)])
def test_attention_calls_of_the_model(dev, monkeypatch, model, path, l2):
    """Every attention call of a one-block GenerationBatch over its ten steps, checked on the spot against the bound: q as
    the qkv kernels leave it (l2-normalized and scaled under attn_l2_norm) and the cache's fake-quantized K / V."""
    from fpqvar_amd import ops, var_block
    real = ops.attention_blhc
    worst, bad, n = {}, [], []

    def recording(q, k, v, scale):
        out = real(q, k, v, scale)
        key = f"{model} {path} l2={l2} Lkv={k.shape[1]}"
        rat = _note(worst, key, out, am.reference(q, k, v, scale))
        if not rat <= 1.0:
            bad.append((key, tuple(q.shape), rat))
        n.append(k.shape[1])
        return out

    monkeypatch.setattr(ops, "attention_blhc", recording)
    gb = var_block.GenerationBatch(model, "w4a4", depth=1, batch_rows=2, device=dev, seed=4, attn_l2_norm=l2)
    caches = gb.new_caches(path)
    for pn in gb.patch_nums:
        assert torch.isfinite(gb.step(path, caches, gb.new_input(pn))).all()
    assert n == [Lkv for _, _, Lkv in am.model_calls(gb.patch_nums, gb.H)]
    _report(f"{model} path {path} attn_l2_norm={l2}", worst, bad)
