"""Generate tests/golden/reference_blocks*.npz by EXECUTING the reference's own AdaLNSelfAttn blocks on the CPU.

Run in the build container only (needs /root/reference); it does not touch reference_vectors.npz:

    python tests/golden/make_block_golden.py

The reference is imported under the two stub modules of make_golden.py (`quant_cuda.quant` = oracle.fpq_oracle.nearest_kernel, `dist`);
everything else - the block, the attention wiring with its KV cache, the Linears, the quantizers' scale arithmetic, transform_model,
rotate_model and quantize_VAR - is the reference's code running.  Each regime is a model of depth 2 whose blocks hold the same
weights (GenerationBatch and BlockModel share one set), run over 2 rows and the first three scale steps (1, 4, 9 tokens) with
kv_caching(True), quant_KV=True, kv_bit=6, flash_if_available=False, fused_if_available=False, `ada_lin` replaced by a module that
returns recorded modulation, and an fp16 residual stream between blocks under the driver's fp16 autocast (fp32 without it).

One difference between the driver's CUDA autocast and the CPU autocast here is removed, one stays:
  * CUDA autocast runs layer_norm in fp32; the CPU one would run it in the stream's fp16.  A forward pre-hook on `ln_wo_grad` casts
    its input to fp32, which is what the CUDA policy does.
  * softmax: fp32 under CUDA autocast, the scores' fp16 here.  `slow_attn` calls it as a tensor method; it stays, and is part of the
    recorded run's distance from the float64 model.

Regimes (tests/test_block_reference_host.py reads them by these names):
  A  C = 1920, 30 heads, block rotation, s = rand + 0.5:  w4a4, w4a4+l2, w6a6, w6a6+l2, and w4a4/fp32, w4a4+l2/fp32 (no autocast;
     W6A6 cannot run in fp32: its quantizer hard-casts to fp16 and the Linear refuses the dtype mix)
  B  as A with the learned vectors of VAR-d30: s_qkv the mat_qkv block holding the file's maximum, s_fc1 the fc1 block holding the
     file's minimum;  w4a4+l2, w6a6+l2
  C  C = 2304, 36 heads, the learned vectors of VAR-d36, block 0 of both files (fc1: four negative entries, min |s| 0.012);
     w4a4+l2, w6a6+l2, and w4a4+l2/fp32 (the run that shows whether the model reads negative and tiny factors as the reference does,
     undisturbed by fp16 noise)
  D  C = 1920, rotate_model(model, "cpu", False) (the dense randomized Hadamard matrix), s = rand + 0.5:  w4a4, w6a6

Files (each below the repository's 1 MiB limit; the loader tests/block_fixture.py merges them):
  reference_blocks.npz         everything but the step outputs: per width the step inputs and the modulation (the same recorded
                               modulation serves every regime of a width), per family the two smoothing vectors, per regime
                               scale_mul_1H11 / q_bias / v_bias, the weights' construction and SHA-256 sums, the learned vectors
  reference_blocks_out_<F>.npz the step outputs of family F's regimes

Weights are not stored.  tests/block_fixture.py's `raw_weight` makes them in integer arithmetic (a 32-bit mixing function of the element index, four bytes
summed: Irwin-Hall, standard deviation 0.02), so a test repeats them exactly; the fixture holds the SHA-256 of every raw weight and
of every weight as the reference's Linears hold it after transform_model, rotate_model and quantize_VAR.

The zip members carry a fixed timestamp: two runs write the same bytes.
"""
import functools
import hashlib
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = "/root/reference"

DEPTH, ROWS, PATCH_NUMS = 2, 2, (1, 2, 3)
WIDTHS = {1920: 30, 2304: 36}
WEIGHT_SEEDS = {"qkv": 1, "proj": 2, "fc1": 3, "fc2": 4}
WEIGHT_STD = 0.02
FAMILIES = {          # family -> (C, block_rotate, where its smoothing vectors come from)
    "A": (1920, True, "drawn"),
    "B": (1920, True, "var30"),
    "C": (2304, True, "var36"),
    "D": (1920, False, "drawn"),
}
REGIMES = [           # (family, config, attn_l2_norm, autocast)
    ("A", "w4a4", False, True), ("A", "w4a4", True, True), ("A", "w6a6", False, True), ("A", "w6a6", True, True),
    ("A", "w4a4", False, False), ("A", "w4a4", True, False),
    ("B", "w4a4", True, True), ("B", "w6a6", True, True),
    ("C", "w4a4", True, True), ("C", "w6a6", True, True), ("C", "w4a4", True, False),
    ("D", "w4a4", False, True), ("D", "w6a6", False, True),
]
RUN_CFGS = {          # run.sh, as make_golden.py has them
    "w4a4": dict(weight_quant="per_group", act_quant="per_group", w_bit=4, a_bit=4, act_quant_sym=True,
                 activation_fp_quant=True, weight_fp_quant=True, act_fp_type="fp_e2", weight_fp_type="fp_e2",
                 fc2_fp_type="fp_e1m2_neg_e2m1_pos"),
    "w6a6": dict(weight_quant="per_channel", act_quant="per_token", w_bit=6, a_bit=6, act_quant_sym=True,
                 activation_fp_quant=True, weight_fp_quant=True, act_fp_type="fp6_e2m3",
                 weight_fp_type="fp6_e2m3", fc2_fp_type="fp6_int_neg_e2m3_pos"),
}


def sha256(t: torch.Tensor) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(t.detach().contiguous().numpy().tobytes()).digest(), dtype=np.uint8).copy()


def save_npz(path: str, arrays: dict) -> None:
    """np.savez_compressed with a fixed member timestamp and order"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, REFERENCE)
    from oracle import fpq_oracle as orc
    from tests.block_fixture import raw_weight, regime_name, weight_shapes          # shared with the tests that rebuild the weights

    qc = types.ModuleType("quant_cuda")
    qc.quant = lambda x, y: (orc.nearest_kernel(x, y), torch.zeros_like(x))
    sys.modules["quant_cuda"] = qc
    dist = types.ModuleType("dist")
    dist.get_device = lambda: "cpu"
    dist.initialized = lambda: False
    sys.modules["dist"] = dist
    sys.modules.setdefault("quant_utils", types.ModuleType("quant_utils"))

    import models_fp_quant_transform_rotate.quant_utils as qu
    import models_fp_quant_transform_rotate.basic_var as bv
    from rotate_utils import rotation_utils as ru
    import learnable_transformation.transform_model_utils as tmu

    class Recorded(torch.nn.Module):
        """stands in for a block's ada_lin: the recorded modulation [B, 1, 6, C], fp16 as the driver's autocast Linear gives it"""

        def __init__(self, mods, as_fp32):
            super().__init__()
            self.mods, self.as_fp32 = mods, as_fp32

        def forward(self, cond):
            return torch.stack([t.float() if self.as_fp32 else t for t in self.mods], dim=2)

    class Toy(torch.nn.Module):
        def __init__(self, C, H, l2):
            super().__init__()
            self.C = C
            self.blocks = torch.nn.ModuleList([
                bv.AdaLNSelfAttn(block_idx=i, last_drop_p=0, embed_dim=C, cond_dim=8, shared_aln=False,
                                 norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6), num_heads=H, attn_l2_norm=l2,
                                 flash_if_available=False, fused_if_available=False) for i in range(DEPTH)])

    out = {"meta/depth": np.array(DEPTH), "meta/rows": np.array(ROWS), "meta/patch_nums": np.array(PATCH_NUMS),
           "meta/weight_std": np.array(WEIGHT_STD), "meta/regimes": np.array([regime_name(*r) for r in REGIMES])}
    for name, seed in WEIGHT_SEEDS.items():
        out[f"meta/weight_seed/{name}"] = np.array(seed)

    # ---- per width: step inputs, modulation, raw weights ---------------------------------------------------------------------
    xs, mods, raw = {}, {}, {}
    for C, H in WIDTHS.items():
        g = torch.Generator().manual_seed(1000 + C)
        mods[C] = [[(torch.randn(ROWS, 1, C, generator=g) * 0.2).half() for _ in range(6)] for _ in range(DEPTH)]
        xs[C] = [torch.randn(ROWS, pn * pn, C, generator=g).half() for pn in PATCH_NUMS]
        raw[C] = {n: raw_weight(WEIGHT_SEEDS[n], o, i, WEIGHT_STD) for n, (o, i) in weight_shapes(C).items()}
        out[f"width/{C}/heads"] = np.array(H)
        out[f"width/{C}/mods"] = torch.stack([torch.stack(m) for m in mods[C]]).numpy()          # [depth, 6, B, 1, C] fp16
        for i, x in enumerate(xs[C]):
            out[f"width/{C}/x{i}"] = x.numpy()
        for n, w in raw[C].items():
            out[f"width/{C}/raw_sha256/{n}"] = sha256(w)

    # ---- the learned vectors that are used, as data -----------------------------------------------------------------------------
    learned = {}
    for tag in ("var30", "var36"):
        files = {n: torch.stack([t.detach().float() for t in torch.load(
            os.path.join(REFERENCE, "learnable_transformation", f"best_lambda_{tag}", f"{n}_best_s_fp4.pt"), map_location="cpu")])
            for n in ("mat_qkv", "fc1")}
        if tag == "var30":
            pick = {"mat_qkv": int(files["mat_qkv"].max(dim=1)[0].argmax()), "fc1": int(files["fc1"].abs().min(dim=1)[0].argmin())}
        else:
            pick = {"mat_qkv": 0, "fc1": 0}
        for n, b in pick.items():
            learned[tag, n] = files[n][b].clone()
            out[f"learned/{tag}/{n}"] = learned[tag, n].numpy()
            out[f"learned/{tag}/{n}/block"] = np.array(b)

    # ---- per family: the two smoothing vectors ----------------------------------------------------------------------------------
    smooth = {}
    for fam, (C, _, source) in FAMILIES.items():
        if source == "drawn":
            g = torch.Generator().manual_seed(2000 + C)          # A and D: the same drawn vectors
            smooth[fam] = (torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5)
        else:
            smooth[fam] = (learned[source, "mat_qkv"], learned[source, "fc1"])
        out[f"family/{fam}/C"], out[f"family/{fam}/block_rotate"] = np.array(C), np.array(FAMILIES[fam][1])
        out[f"family/{fam}/s_qkv"], out[f"family/{fam}/s_fc1"] = smooth[fam][0].numpy(), smooth[fam][1].numpy()

    # ---- the regimes ---------------------------------------------------------------------------------------------------------------
    outputs = {fam: {} for fam in FAMILIES}
    for fam, config, l2, autocast in REGIMES:
        name = regime_name(fam, config, l2, autocast)
        C, block_rotate, _ = FAMILIES[fam]
        H = WIDTHS[C]
        toy = Toy(C, H, l2).eval()
        g = torch.Generator().manual_seed(3000 + C)          # one draw of the l2 parameters per width
        with torch.no_grad():
            for b in toy.blocks:
                for n, lin in (("qkv", b.attn.mat_qkv), ("proj", b.attn.proj), ("fc1", b.ffn.fc1), ("fc2", b.ffn.fc2)):
                    lin.weight.copy_(raw[C][n])
                    if lin.bias is not None:
                        lin.bias.zero_()          # GenerationBatch has no Linear biases
                if l2:
                    sm = torch.full((1, H, 1, 1), 4.0).log() + 0.3 * torch.randn(1, H, 1, 1, generator=g)
                    sm[0, 0] = b.attn.max_scale_mul + 0.5          # head 0 above the clamp, as GenerationBatch draws it
                    b.attn.scale_mul_1H11.copy_(sm)
                    b.attn.q_bias.copy_(torch.randn(C, generator=g) * 0.1)
                    b.attn.v_bias.copy_(torch.randn(C, generator=g) * 0.1)
                b.ln_wo_grad.register_forward_pre_hook(lambda mod, args: (args[0].float(),))          # CUDA autocast's layer_norm
        s_qkv, s_fc1 = smooth[fam]
        tmu.transform_model(toy, [s_qkv] * DEPTH, [s_fc1] * DEPTH)
        ru.rotate_model(toy, "cpu", block_rotate)
        qu.quantize_VAR(toy, **RUN_CFGS[config])
        if block_rotate:
            Q = ru.block_random_hadamard_matrix(C, 128, "cpu", 42).to(torch.float32)
        else:
            Q = ru.get_orthogonal_matrix(C, "hadamard", "cpu").to(torch.float32)          # evaluate_fp_quant_transform_rotate.py:143
        for b in toy.blocks:
            b.attn.kv_caching(True)
        ys = []
        for si, x in enumerate(xs[C]):
            x = x if autocast else x.float()
            for i, b in enumerate(toy.blocks):
                b.ada_lin = Recorded(mods[C][i], not autocast)
                with torch.no_grad(), torch.autocast("cpu", dtype=torch.float16, enabled=autocast):
                    x = b(x, None, None, si, True, 6, Q, s_qkv, s_fc1)
                if autocast:
                    x = x.half()          # the fp16 residual stream
            assert x.dtype == (torch.float16 if autocast else torch.float32) and bool(torch.isfinite(x).all()), name
            ys.append(x)
        for i, y in enumerate(ys):
            outputs[fam][f"out/{name}/y{i}"] = y.numpy()
        b0 = toy.blocks[0]
        for n, lin in (("qkv", b0.attn.mat_qkv), ("proj", b0.attn.proj), ("fc1", b0.ffn.fc1), ("fc2", b0.ffn.fc2)):
            w = lin.weight.detach()
            assert torch.equal(w, dict(qkv=toy.blocks[1].attn.mat_qkv, proj=toy.blocks[1].attn.proj, fc1=toy.blocks[1].ffn.fc1,
                                       fc2=toy.blocks[1].ffn.fc2)[n].weight)
            # as the Linear multiplies it: fp16 under autocast, the quantizer's own dtype without
            out[f"regime/{name}/weight_sha256/{n}"] = sha256(w.half() if autocast else w)
            out[f"regime/{name}/weight_dtype/{n}"] = np.array(str(w.dtype))
        if l2:
            out[f"regime/{name}/scale_mul"] = torch.stack([b.attn.scale_mul_1H11.detach() for b in toy.blocks]).numpy()
            out[f"regime/{name}/q_bias"] = torch.stack([b.attn.q_bias.detach() for b in toy.blocks]).numpy()
            out[f"regime/{name}/v_bias"] = torch.stack([b.attn.v_bias.detach() for b in toy.blocks]).numpy()
        print(name, [tuple(y.shape) for y in ys], ys[0].dtype, flush=True)

    save_npz(os.path.join(HERE, "reference_blocks.npz"), out)
    for fam, arrays in outputs.items():
        save_npz(os.path.join(HERE, f"reference_blocks_out_{fam}.npz"), arrays)
    for f in ["reference_blocks.npz"] + [f"reference_blocks_out_{fam}.npz" for fam in FAMILIES]:
        print("wrote", f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
