"""GPU: the fused form of the format search (search_layer(fused=True), search_layers_fused, search_blocks_sharded_fused) against
the sample-by-sample loop and the default batched form: same winners, losses within the 2e-3 the existing contract
(tests/test_gpu_configs.py::test_config4_format_search_d30_layer) demands between the forms - the stacked GEMM has another M and
the vendor library may choose another kernel, so nothing tighter is claimed for the whole function."""
import pytest
import torch

pytestmark = pytest.mark.gpu

REL = 2e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _small_layer(dev, seed=0, dtype=torch.float16):
    """w [384 x 256], 10 samples of [2, pn^2, 256] for pn = 1 .. 5 twice; heavy-tailed like pre-quantization activations"""
    g = torch.Generator(device=dev).manual_seed(900 + seed)
    xs = []
    for j in range(10):
        shape = (2, (j % 5 + 1) ** 2, 256)
        xs.append((torch.randn(shape, device=dev, generator=g) * torch.exp(0.5 * torch.randn(shape, device=dev, generator=g))).half())
    w = (torch.randn(384, 256, device=dev, generator=g) * 0.02).to(dtype)
    return xs, w


def _config4_layer(dev, block=0, n=100):
    """One d30 mat_qkv layer and its calibration dump, generated as tests/test_gpu_configs.py::_config4_search_layer does:
    w [5760 x 1920], 100 samples x_j [2, pn^2, 1920] over the ten scale steps, 13600 rows in all."""
    g = torch.Generator(device=dev).manual_seed(400 + block)
    pns = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
    xs = []
    for j in range(n):
        shape = (2, pns[j % 10] ** 2, 1920)
        xs.append((torch.randn(shape, device=dev, generator=g) * torch.exp(0.5 * torch.randn(shape, device=dev, generator=g))).half())
    w = (torch.randn(5760, 1920, device=dev, generator=g) * 0.02).half()
    return xs, w


def _agree(fused, other, formats):
    (wf, af, lf), (wo, ao, lo) = fused, other
    assert set(lf) == set(lo) and len(lf) == len(formats) ** 2
    for key in lo:
        print(f"{key}: fused {lf[key]:.8g} other {lo[key]:.8g} rel {abs(lf[key] - lo[key]) / lo[key]:.3g}")
        assert abs(lf[key] - lo[key]) <= REL * lo[key], (key, lf[key], lo[key])
    assert (wf, af) == (wo, ao)


@pytest.mark.parametrize("dtype", (torch.float16, torch.float32), ids=("w16", "w32"))
def test_fused_layer_against_the_sample_loop(dev, dtype):
    from fpqvar_amd import format_search as fs
    xs, w = _small_layer(dev, 0, dtype)
    for formats in (fs.FP6_FORMATS, fs.FP4_FORMATS):
        _agree(fs.search_layer(xs, w, formats, fused=True), fs.search_layer(xs, w, formats, batched=False), formats)
    # the default is the batched form, whether `fused` is named or not
    a, b = fs.search_layer(xs, w, fs.FP4_FORMATS), fs.search_layer(xs, w, fs.FP4_FORMATS, fused=False)
    _agree(a, b, fs.FP4_FORMATS)
    with pytest.raises(RuntimeError, match="float16 or float32"):
        fs.search_layer(xs, w.double(), fs.FP6_FORMATS, fused=True)


def test_layers_fused_is_the_layers_one_by_one_and_does_not_synchronise(dev):
    from fpqvar_amd import format_search as fs
    layers = [_small_layer(dev, s) for s in range(3)]
    for formats in (fs.FP6_FORMATS, fs.FP4_FORMATS):
        nf = len(formats)
        fs.search_layers_fused(layers[:1], formats)                                 # the row weights of this calibration set are in place
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            table = fs.search_layers_fused(iter(layers), formats)
            one = torch.empty(nf, nf, dtype=torch.float32, device=dev)
            assert fs.search_layer(*layers[0], formats, fused=True, losses_out=one) is None
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert table.shape == (3, nf, nf) and table.dtype == torch.float32 and table.is_cuda
        host = table.cpu()
        for k, (xs, w) in enumerate(layers):
            wf, af, losses = fs.search_layer(xs, w, formats, fused=True)
            want = torch.tensor([[losses[(a, b)] for b in formats] for a in formats], dtype=torch.float32)
            assert torch.equal(host[k].view(torch.int32), want.view(torch.int32)), k
            assert fs.pick_winner(host[k], formats) == (wf, af)
        assert torch.equal(one.cpu().view(torch.int32), host[0].view(torch.int32))


def test_sharded_fused_at_world_one(dev):
    from fpqvar_amd import format_search as fs
    layers = [_small_layer(dev, s) for s in range(3)]
    for formats in (fs.FP6_FORMATS, fs.FP4_FORMATS):
        def evaluate(b):
            wf, af, losses = fs.search_layer(*layers[b], formats, fused=True)
            return wf, af, losses[(wf, af)]
        want = fs.search_blocks_sharded(3, evaluate, formats)
        got = fs.search_blocks_sharded_fused(3, lambda b: layers[b], formats)
        assert got == want, (got, want)
    assert fs.search_blocks_sharded_fused(0, lambda b: layers[b], fs.FP6_FORMATS) == []


def test_config4_size_against_the_default_batched_form(dev):
    from fpqvar_amd import format_search as fs
    xs, w = _config4_layer(dev)
    assert sum(x.numel() // 1920 for x in xs) == 13600
    _agree(fs.search_layer(xs, w, fs.FP4_FORMATS, fused=True), fs.search_layer(xs, w, fs.FP4_FORMATS), fs.FP4_FORMATS)
