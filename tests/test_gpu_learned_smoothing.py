"""The producers under the smoothing vectors the reference ships.  Every other test draws the vector from rand * 1.5 + 0.25 or
rand + 0.5; the learned ones (tests/golden/reference_blocks.npz: VAR-d30 mat_qkv with the file's maximum 2.79, VAR-d30 fc1 with its
minimum 0.050, VAR-d36 mat_qkv and fc1 of block 0 - the latter with four NEGATIVE factors and one of 0.012) reach five places that
have never seen such a factor: the A / B fold of the adaLN producers, the widening fma of rotate_quant, the LDS-staged vector of the
block rotation, and the two full-width row loads.

17 rows per case (every row family of tests/adaln_model.py, one batch entry of odd length), each vector at its own width, fp16 and
fp32 rows.

  h         adaln_rotate_quant, its gated-residual form and adaln_rotate_quant_full put the modulated row within adaln_model.bound /
            fulladaln_model.bound of the float64 reference (the bounds are fair under these vectors: the fp32 models of the kernels
            stay within them, test_adaln_model_host.py / test_fulladaln_model_host.py); the per-token forms, which do not return h,
            give bit for bit the per-token quantization of the emitting form's rotated row.
  rotation  rotate_quant(x, smooth=s) is rotate_quant(half(float(x) * s)) bit for bit - values, rotated row, FP4 operands; the
            rotated rows of rotate_quant_full are within fullrot_model.bound of the float64 product.
  zeros     a zero element under a negative factor carries the sign the reference's torch chain gives it.
"""
import pytest
import torch

from tests import adaln_model as am
from tests import block_fixture as bf
from tests import fulladaln_model as fa
from tests import fullrot_model as fr

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
VECTORS = ("var30/mat_qkv", "var30/fc1", "var36/mat_qkv", "var36/fc1")
ROWS, EPS = 17, 1e-6
CASES = [(v, xd) for v in VECTORS for xd in (F16, F32)]
IDS = [f"{v.replace('/', '-')}-{str(xd)[6:]}" for v, xd in CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def _case(dev, vector, x_dtype, mod_dtype=F16):
    """(x [1, 17, C], scale, shift [1, C], smooth [C]) on the GPU: adaln_model's rows under a learned vector"""
    smooth = bf.learned_vectors()[vector]
    C = smooth.numel()
    x, scale, shift, _ = am.make_case(1, ROWS, C, x_dtype, mod_dtype, False, EPS)
    assert set(am.families(ROWS, C)) == set(am.FAMILIES)
    return x.view(1, ROWS, C).to(dev), scale.to(dev), shift.to(dev), smooth.to(dev), C


def _bits(t):
    """fp16 -> int16 bit patterns with every NaN one value (signed zeros stay apart)"""
    assert t.dtype == F16
    return torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t).contiguous().view(torch.int16)


def _same(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _check_h(model, h, x, scale, shift, smooth, x_dtype, C, what):
    ref = model.reference(x.view(-1, C).cpu(), scale.cpu(), shift.cpu(), smooth.cpu(), EPS, ROWS)
    assert float(ref["h"][ref["finite"]].abs().max()) < 6.0e4
    worst, where_ok = model.check(h.view(-1, C).cpu(), ref, x_dtype, C)
    print(f"\n{what}: worst err / bound {worst:.4f}")
    assert where_ok, f"{what}: non-finite elements are not where the reference has them"
    assert worst <= 1.0, f"{what}: h beyond the bound, worst err / bound {worst:.3f}"


@pytest.mark.parametrize("vector,x_dtype", CASES, ids=IDS)
def test_modulated_row_of_the_block_producers(dev, vector, x_dtype):
    from fpqvar_amd import ops, rotation as rot
    for mod_dtype in (F16, F32):
        x, scale, shift, smooth, C = _case(dev, vector, x_dtype, mod_dtype)
        what = f"{vector} x={str(x_dtype)[6:]} mod={str(mod_dtype)[6:]}"
        out, h, y = rot.adaln_rotate_quant(x, scale, shift, "e2m1", smooth=smooth, eps=EPS, return_intermediates=True)
        _check_h(am, h, x, scale, shift, smooth, x_dtype, C, f"adaln_rotate_quant {what}")
        tok = rot.adaln_rotate_quant_token(x, scale, shift, "e2m3", smooth=smooth, eps=EPS)
        assert _same(tok, ops.quant_rows(y, "e2m3", C, F16)), f"adaln_rotate_quant_token {what}: not the quantized rotated row of the emitting form"

        # the gated-residual forms: x = residual + y_in * gate, then the same producer
        g = torch.Generator().manual_seed(C + 5)
        y_in = (torch.randn(1, ROWS, C, generator=g) * 0.5).half().to(dev)
        gate = (torch.randn(1, C, generator=g) * 0.3).half().to(dev)
        x_new, r_out, r_h, r_y = rot.resid_adaln_rotate_quant(y_in, gate, x, scale, shift, "e2m1", smooth=smooth, eps=EPS,
                                                              return_intermediates=True)
        want_x = x + y_in.mul(gate.view(1, 1, C))
        assert x_new.dtype == x_dtype and bool(((x_new == want_x) | (torch.isnan(x_new) & torch.isnan(want_x))).all()), f"resid {what}: x_new"
        _check_h(am, r_h, x_new, scale, shift, smooth, x_dtype, C, f"resid_adaln_rotate_quant {what}")
        _, r_tok = rot.resid_adaln_rotate_quant_token(y_in, gate, x, scale, shift, "e2m3", smooth=smooth, eps=EPS)
        assert _same(r_tok, ops.quant_rows(r_y, "e2m3", C, F16)), f"resid_adaln_rotate_quant_token {what}: not the quantized rotated row"


@pytest.mark.parametrize("vector,x_dtype", CASES, ids=IDS)
def test_modulated_and_rotated_row_of_the_full_width_producer(dev, vector, x_dtype):
    from fpqvar_amd import rotation as rot
    for mod_dtype in (F16, F32):
        x, scale, shift, smooth, C = _case(dev, vector, x_dtype, mod_dtype)
        what = f"{vector} x={str(x_dtype)[6:]} mod={str(mod_dtype)[6:]}"
        out, h, y = rot.adaln_rotate_quant_full(x, scale, shift, "e2m1", smooth=smooth, eps=EPS, return_intermediates=True)
        _check_h(fa, h, x, scale, shift, smooth, x_dtype, C, f"adaln_rotate_quant_full {what}")
        _check_rotated(h.view(-1, C).cpu(), y.view(-1, C).cpu(), C, f"adaln_rotate_quant_full {what}")


def _check_rotated(h16, y, C, what):
    """the rows of h16 that are finite: y within fullrot_model.bound of float64(h16) @ Q"""
    fin = torch.isfinite(h16).all(dim=1)
    ref = fr.reference(h16[fin], C)
    ratio = ((y[fin].double() - ref).abs() / fr.bound(h16[fin], ref, C))
    worst = float(torch.nan_to_num(ratio, nan=float("inf")).max())
    print(f"{what}: rotated row, worst err / bound {worst:.4f} over {int(fin.sum())} finite rows")
    assert worst <= 1.0, f"{what}: rotated row beyond fullrot_model.bound, worst err / bound {worst:.3f}"
    assert not bool(torch.isfinite(y[~fin]).all(dim=1).any()), f"{what}: a non-finite row came out finite"


def _plain_rows(vector, x_dtype):
    """adaln_model's 17 rows as the rotation's input (the 1e4 family overflows to inf under a factor of 2.79: compared as such)"""
    smooth = bf.learned_vectors()[vector]
    C = smooth.numel()
    x = am.make_rows(ROWS, C, x_dtype, EPS)
    return x, smooth, C


@pytest.mark.parametrize("vector,x_dtype", CASES, ids=IDS)
def test_block_rotation_folds_the_vector_as_the_torch_chain(dev, vector, x_dtype):
    """rotate_quant(x, smooth=s) against rotate_quant(half(float(x) * s)): values, rotated row and FP4 operands (row-major and
    k-major), bit for bit - NaNs one value, overflow to inf at 1e4 * 2.79 included."""
    from fpqvar_amd import rotation as rot
    x, smooth, C = _plain_rows(vector, x_dtype)
    folded = (x.float() * smooth).half()
    xd, sd, fd = x.to(dev), smooth.to(dev), folded.to(dev)
    for table in ("e2m1", "e2m3"):
        out, y = rot.rotate_quant(xd, table, smooth=sd, return_rotated=True)
        want, want_y = rot.rotate_quant(fd, table, return_rotated=True)
        assert _same(y, want_y), f"{vector} {table}: rotated rows differ"
        assert _same(out, want), f"{vector} {table}: values differ"
    for km in (False, True):
        codes, scales = rot.rotate_quant_mx(xd, smooth=sd, kmajor=km)
        want_codes, want_scales = rot.rotate_quant_mx(fd, kmajor=km)
        assert torch.equal(codes, want_codes), f"{vector}: FP4 operand codes differ (kmajor={km})"
        nan = torch.isnan(scales)          # the scales of a non-finite row
        assert torch.equal(nan, torch.isnan(want_scales)) and torch.equal(scales[~nan], want_scales[~nan]), \
            f"{vector}: FP4 operand scales differ (kmajor={km})"


@pytest.mark.parametrize("vector,x_dtype", CASES, ids=IDS)
def test_full_width_rotation_under_the_learned_vectors(dev, vector, x_dtype):
    """rotate_quant_full(x, smooth=s): the rotated rows within fullrot_model.bound of float64(half(float(x) * s)) @ Q, and bit for
    bit the rotated rows of the folded input; the same for fullrot_model's own four row families."""
    from fpqvar_amd import rotation as rot
    x, smooth, C = _plain_rows(vector, x_dtype)
    rows = [("adaln rows", x)] + [(name, make(ROWS, C).to(x_dtype)) for name, make in fr.FAMILIES.items()]
    for name, xr in rows:
        folded = (xr.float() * smooth).half()
        out, y = rot.rotate_quant_full(xr.to(dev), "e2m1", smooth=smooth.to(dev), return_rotated=True)
        _check_rotated(folded, y.cpu(), C, f"rotate_quant_full {vector} {name}")
        want, want_y = rot.rotate_quant_full(folded.to(dev), "e2m1", return_rotated=True)
        assert _same(y, want_y) and _same(out, want), f"{vector} {name}: not the rotation of the folded rows"


@pytest.mark.parametrize("x_dtype", (F16, F32), ids=("float16", "float32"))
def test_signed_zeros_under_negative_factors(dev, x_dtype):
    """A zero row has LN(x) = +0 exactly, so the reference's torch chain gives h = (0 * (scale + 1) + shift) * s = shift * s.  Where
    shift is +0 that is -0 under a negative factor and +0 under a positive one, and the kernels' h must carry exactly these bits,
    as on every non-zero element of the row.  VAR-d36's fc1 vector: channels 515, 532, 600, 619 are negative.

    Where shift is -0 (channels 532, 1, 8 here) the chain adds first, (+0) + (-0) = +0, and then takes the factor's sign.  The
    kernels fold s - and the rotation's sign vector D - into A = (scale + 1) s D and B = shift s D and compute fma(LN, A, B), the sum
    of two zeros whose signs the fold has changed one by one; the sign of that sum is the chain's only by chance.  Measured on an
    MI355X: adaln_rotate_quant gives +0 at channel 532 (the chain: -0) and -0 at channel 8 (the chain: +0, D[8] = -1),
    adaln_rotate_quant_full +0 at channel 532; channel 1 agrees.  An fp16 -0 in a Linear's output does not occur in practice and
    the sign of a zero in h reaches no output (the rotation adds it to the row's other elements), so for these elements the test
    asserts the value, prints the sign differences, and the arithmetic stays as it is."""
    from fpqvar_amd import rotation as rot
    import torch.nn.functional as Fn
    smooth = bf.learned_vectors()["var36/fc1"]
    C = smooth.numel()
    assert (smooth < 0).nonzero().flatten().tolist() == [515, 532, 600, 619]
    plus_zero, minus_zero = [515, 619, 0, 7], [532, 1, 8]
    g = torch.Generator().manual_seed(4)
    x = torch.zeros(2, 3, C, dtype=x_dtype)
    scale = (torch.randn(2, C, generator=g) * 0.3).half()
    shift = (torch.randn(2, C, generator=g) * 0.3).half()
    shift[:, plus_zero] = 0.0
    shift[:, minus_zero] = -0.0
    chain = Fn.layer_norm(x.float(), (C,), eps=EPS).mul(scale.add(1).view(2, 1, C)).add_(shift.view(2, 1, C)).mul(smooth).half()
    assert bool((chain[:, :, plus_zero + minus_zero] == 0).all())
    assert bool(torch.signbit(chain[:, :, [515, 619, 532]]).all()) and not bool(torch.signbit(chain[:, :, [0, 7, 1, 8]]).any())
    xd, scd, shd, sd = x.to(dev), scale.to(dev), shift.to(dev), smooth.to(dev)
    got = {"adaln_rotate_quant": rot.adaln_rotate_quant(xd, scd, shd, "e2m1", smooth=sd, eps=EPS, return_intermediates=True)[1],
           "adaln_rotate_quant_full": rot.adaln_rotate_quant_full(xd, scd, shd, "e2m1", smooth=sd, eps=EPS, return_intermediates=True)[1]}
    strict = torch.ones(C, dtype=torch.bool)
    strict[minus_zero] = False
    bad = {}
    for name, h in got.items():
        h = h.cpu()
        diff = (_bits(h) != _bits(chain)).nonzero()
        channels = sorted(set(diff[:, 2].tolist()))
        print(f"\n{name} x={str(x_dtype)[6:]}: {len(diff)} elements differ from the torch chain in their bits, channels {channels[:12]}")
        assert bool((h[:, :, minus_zero] == 0).all()), f"{name}: a zero element is not zero"
        if [c for c in channels if strict[c]]:
            bad[name] = [c for c in channels if strict[c]][:12]
    assert not bad, f"h differs from the reference's torch chain on a zero row: {bad}"
