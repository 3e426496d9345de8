"""tests/golden/reference_blocks*.npz - the reference's own AdaLNSelfAttn blocks, executed by tests/golden/make_block_golden.py - as
the tests read it: the regimes with their inputs, recorded outputs and parameters, and the weights, which the fixture does not
store: `raw_weight` repeats their construction in integer arithmetic and every tensor is checked against the recorded SHA-256.
CPU only; nothing here touches the product except fpqvar_amd.rotation's weight-side preprocessing."""
import functools
import hashlib
import os
from types import SimpleNamespace

import numpy as np
import torch

from oracle import fpq_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAMILIES = ("A", "B", "C", "D")
WEIGHT_NAMES = ("qkv", "proj", "fc1", "fc2")


def regime_name(family, config, l2, autocast=True):
    return f"{family}/{config}{'+l2' if l2 else ''}{'' if autocast else '/fp32'}"


def weight_shapes(C: int):
    return {"qkv": (3 * C, C), "proj": (C, C), "fc1": (4 * C, C), "fc2": (C, 4 * C)}


def raw_weight(seed: int, out_features: int, in_features: int, std: float) -> torch.Tensor:
    """fp32 [out, in]: element i (row-major) is (b0 + b1 + b2 + b3 - 510) * float32(std / sigma), b* the four bytes of a 32-bit mix
    of i and the matrix's seed, sigma = sqrt((256^2 - 1) / 3) the standard deviation of the sum (Irwin-Hall, four terms).  Integer
    arithmetic up to one fp32 multiplication of an exactly representable integer: the same bits on every machine."""
    m32 = 0xFFFFFFFF
    h = (torch.arange(out_features * in_features, dtype=torch.int64) * 2654435761 + seed * 40503) & m32
    h = ((h ^ (h >> 15)) * 2246822519) & m32
    h = ((h ^ (h >> 13)) * 3266489917) & m32
    h = h ^ (h >> 16)
    total = (h & 255) + ((h >> 8) & 255) + ((h >> 16) & 255) + ((h >> 24) & 255) - 510
    unit = torch.tensor(std / ((256.0 ** 2 - 1.0) / 3.0) ** 0.5, dtype=torch.float32)
    return (total.to(torch.float32) * unit).view(out_features, in_features)


def sha256(t: torch.Tensor) -> bytes:
    return hashlib.sha256(t.detach().contiguous().numpy().tobytes()).digest()


@functools.lru_cache(maxsize=None)
def load() -> dict:
    """every array of the fixture's files under its key"""
    data = {}
    for f in ["reference_blocks.npz"] + [f"reference_blocks_out_{fam}.npz" for fam in FAMILIES]:
        with np.load(os.path.join(GOLDEN, f)) as z:
            data.update({k: z[k] for k in z.files})
    return data


def regime_names():
    return [str(n) for n in load()["meta/regimes"]]


@functools.lru_cache(maxsize=None)
def regime(name: str) -> SimpleNamespace:
    """One recorded run (read-only CPU tensors): xs / ys the step inputs and the reference's outputs, mods per block the six fp16
    modulation tensors, s_qkv / s_fc1 fp32, scale_mul / qkv_bias per block under attn_l2_norm (else None)."""
    d = load()
    t = lambda key: torch.from_numpy(d[key])
    family, cfg = name.split("/")[0], name.split("/")[1]
    config, l2, autocast = cfg.split("+")[0], cfg.endswith("+l2"), not name.endswith("/fp32")
    C = int(d[f"family/{family}/C"])
    depth, steps = int(d["meta/depth"]), len(d["meta/patch_nums"])
    mods = t(f"width/{C}/mods")
    scale_mul = qkv_bias = None
    if l2:
        scale_mul = list(t(f"regime/{name}/scale_mul"))
        qb, vb = t(f"regime/{name}/q_bias"), t(f"regime/{name}/v_bias")
        qkv_bias = [torch.cat((qb[b], torch.zeros(C), vb[b])) for b in range(depth)]
    return SimpleNamespace(
        name=name, family=family, config=config, l2=l2, autocast=autocast, C=C, H=int(d[f"width/{C}/heads"]), depth=depth,
        rows=int(d["meta/rows"]), block_rotate=bool(d[f"family/{family}/block_rotate"]),
        xs=[t(f"width/{C}/x{i}") for i in range(steps)], ys=[t(f"out/{name}/y{i}") for i in range(steps)],
        mods=[[mods[b, j] for j in range(6)] for b in range(depth)], s_qkv=t(f"family/{family}/s_qkv"), s_fc1=t(f"family/{family}/s_fc1"),
        scale_mul=scale_mul, qkv_bias=qkv_bias)


def learned_vectors():
    """name -> fp32 [C]: the four learned smoothing vectors the fixture stores"""
    d = load()
    return {f"{tag}/{n}": torch.from_numpy(d[f"learned/{tag}/{n}"]) for tag in ("var30", "var36") for n in ("mat_qkv", "fc1")}


@functools.lru_cache(maxsize=None)
def raw_weights(C: int):
    """the unquantized fp32 weights of a width, checked against the fixture's sums"""
    d = load()
    w = {n: raw_weight(int(d[f"meta/weight_seed/{n}"]), o, i, float(d["meta/weight_std"])) for n, (o, i) in weight_shapes(C).items()}
    for n, t in w.items():
        assert sha256(t) == d[f"width/{C}/raw_sha256/{n}"].tobytes(), \
            f"cannot reproduce the fixture's raw weight {n} at C = {C}: raw_weight no longer gives the recorded SHA-256"
    return w


@functools.lru_cache(maxsize=None)
def rotation_matrix(C: int, block_rotate: bool) -> torch.Tensor:
    """fp32 Q as the driver passes it to the blocks"""
    from fpqvar_amd import rotation as rot
    q = orc.block_hadamard(C, 128, 42) if block_rotate else rot.get_orthogonal_matrix(C, device="cpu")
    return q.float()


@functools.lru_cache(maxsize=None)
def _quantized(family: str, config: str):
    """the weight quantizer's own output (fp32 for W4A4, fp16 for W6A6) on the transformed and rotated weights of a family"""
    from fpqvar_amd import rotation as rot
    from tests import block_model as bm
    d = load()
    C, block = int(d[f"family/{family}/C"]), bool(d[f"family/{family}/block_rotate"])
    s_qkv, s_fc1 = torch.from_numpy(d[f"family/{family}/s_qkv"]), torch.from_numpy(d[f"family/{family}/s_fc1"])
    q64 = (orc.block_hadamard(C, 128, 42) if block else rot.get_orthogonal_matrix(C, device="cpu")).double()
    w = dict(raw_weights(C))
    w["qkv"] = rot.rotate_weight(rot.transform_weight(w["qkv"], s_qkv), q64)
    w["fc1"] = rot.rotate_weight(rot.transform_weight(w["fc1"], s_fc1), q64)
    quant = (lambda t: orc.per_group_kernel_sem(t, "e2m1", 128)) if config == "w4a4" else bm.CONFIGS["w6a6"]["weight"]
    return {n: quant(t) for n, t in w.items()}


def weights(name: str):
    """The weights as the reference's Linears multiply them in regime `name`: fp16 under autocast, the quantizer's output without.
    Fails - it does not skip - when they do not hash to what the reference held."""
    r, d = regime(name), load()
    w = {n: (t.half() if r.autocast else t) for n, t in _quantized(r.family, r.config).items()}
    for n, t in w.items():
        assert sha256(t) == d[f"regime/{name}/weight_sha256/{n}"].tobytes(), \
            (f"cannot reproduce the weights of regime {name}: {n} after transform, rotation and the oracle's weight quantizer does "
             f"not give the SHA-256 of the tensor the reference's Linear held")
    return w


def params(name: str, **overrides):
    """tests.block_model.BlockParams of a recorded regime"""
    from tests import block_model as bm
    r = regime(name)
    fields = dict(C=r.C, H=r.H, config=r.config, w=weights(name), mods=r.mods, s_qkv=r.s_qkv, s_fc1=r.s_fc1,
                  Q=rotation_matrix(r.C, r.block_rotate), scale_mul=r.scale_mul, qkv_bias=r.qkv_bias, fp32=not r.autocast)
    fields.update(overrides)
    return bm.BlockParams(**fields)
