"""GenerationBatch(tensors=...) takes its parameters from outside; without the keyword nothing may change: the same draws in the
same order, the same bits.  tests/golden/generation_default_parent.npz holds the SHA-256 of the step outputs that the commit before
the keyword gave on an MI355X for default batches on a fixed seed (d30-256, depth 2, 2 rows, seed 3, inputs from generator seed 11,
steps of 1 / 4 / 9 tokens; w4a4 and w6a6 with attn_l2_norm; paths R, F, Q)."""
import hashlib
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generation_default_parent.npz")


@pytest.mark.gpu
@pytest.mark.parametrize("config,l2", [("w4a4", False), ("w6a6", True)], ids=["w4a4", "w6a6+l2"])
def test_default_batch_gives_the_parents_bits(config, l2):
    from fpqvar_amd import var_block
    want = np.load(GOLDEN)
    bad = []
    for path in ("R", "F", "Q"):
        gb = var_block.GenerationBatch("d30-256", config, depth=2, batch_rows=2, device="cuda:0", seed=3, attn_l2_norm=l2)
        gb.gen.manual_seed(11)
        xs = [gb.new_input(pn) for pn in gb.patch_nums[:3]]
        caches = gb.new_caches(path)
        ys = [gb.step(path, caches, x) for x in xs]
        torch.cuda.synchronize()
        for i, y in enumerate(ys):
            key = f"{config}{'+l2' if l2 else ''}/{path}/y{i}"
            if hashlib.sha256(y.cpu().contiguous().numpy().tobytes()).digest() != want[key].tobytes():
                bad.append(key)
    assert not bad, f"a default GenerationBatch no longer gives the bits of the commit before `tensors`: {bad}"


def test_tensors_are_all_or_nothing():
    """refused before any tensor is made (no GPU here)"""
    from fpqvar_amd import var_block
    with pytest.raises(ValueError, match="tensors must hold"):
        var_block.GenerationBatch("d30-256", "w4a4", depth=1, batch_rows=2, device="cpu", tensors={"s_qkv": torch.ones(1920)})
    full = dict(w=dict(qkv=None, proj=None, fc1=None, fc2=None), s_qkv=None, s_fc1=None, mods=None)
    with pytest.raises(ValueError, match="scale_mul"):
        var_block.GenerationBatch("d30-256", "w4a4", depth=1, batch_rows=2, device="cpu", attn_l2_norm=True, tensors=full)
