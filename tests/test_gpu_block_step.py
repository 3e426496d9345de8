"""GenerationBatch.step through its public surface only: which wrappers of ops / gemm / rotation / quant_utils a block calls, in
which order and with which cache-facing integers, and the bit equalities between options that hold by construction.

Shape: "d30-256" with depth 2 (the smallest run in which a pending residual crosses a block), four rows, and the first three scale
steps - 1, 4, 9 tokens: the smallest run in which a cache quantizes one step's entries while older ones stay untouched.
Grid: path F / Q x config x kv_storage x q/k norm off / fused / torch x fuse_residual; on path Q also qkv_to_cache, on path F with the
fp16 cache also sdpa_in_f.  Every case runs once (`_run`); the trace test and the equality tests share its result.

The expected sequences (`_expected`) are spelled here from the case's parameters:
  first producer        the adaLN producer of the path and config - its gated-residual form when a residual is pending
  mat_qkv               path Q: the split GEMM into the block's own cache at (len, L) or into the shared staging slab at (0, L), or the
                        plain GEMM; path F: a torch Linear (not recorded)
  KV step + attention   fp16 cache: kv_cache_step / kv_cache_step_qk_norm quantize [previous step's start, len) and copy the step's k / v
                        to len (after the split GEMM: no copy, and no launch in the first step), then attention over len + L keys;
                        packed cache: the fused norm into the staging slab, attention over n_packed = len entries + L fresh ones, then
                        their pack at pos = len
  proj, fc1, fc2 tail   path F: fake-quantizers around torch Linears; path Q: quantizer + GEMM, producer + fc1 GEMM (W4A4: GELU and
                        fc2's quantizer in its epilogue); gate_residual wherever the tail is not pending
"""
import functools
import hashlib
import itertools

import pytest
import torch

from tests.conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

MODEL, DEPTH, ROWS, STEPS = "d30-256", 2, 4, (1, 2, 3)          # patch sizes 1, 2, 3: 1, 4, 9 tokens
NORMS = ("off", "fused", "torch")


def _cases():
    """(path, config, kv_storage, norm, fuse_residual, qkv_to_cache, sdpa_in_f)"""
    out = []
    for config, storage, norm, fuse in itertools.product(("w4a4", "w6a6"), ("fp16", "codes"), NORMS, (False, True)):
        out.append(("F", config, storage, norm, fuse, True, False))
        if storage == "fp16":
            out.append(("F", config, storage, norm, fuse, True, True))
        out += [("Q", config, storage, norm, fuse, split, False) for split in (True, False)]
    return out


CASES = _cases()


def case_id(case):
    path, config, storage, norm, fuse, split, sdpa = case
    return "-".join((path, config, storage, "norm_" + norm, "fuse" if fuse else "nofuse",
                     *(("split" if split else "copyin",) if path == "Q" else ()), *(("sdpa",) if sdpa else ())))


# ---- the recorders -------------------------------------------------------------------------------------------------------------
def _n(t):
    return int(t.shape[1])


# name -> the cache-facing integers of a call (slab: the tensor whose owner is looked up)
FACING = {
    "kv_cache_step": lambda cache, qs, qe, k, v, new_start, *a, **kw: dict(slab=cache, quant_start=qs, quant_stop=qe, new_start=new_start, n=_n(k)),
    "kv_cache_step_qk_norm": lambda cache, qs, qe, q, k, v, new_start, *a, **kw: dict(slab=cache, quant_start=qs, quant_stop=qe,
                                                                                    new_start=new_start, n=_n(k)),
    "kv_pack": lambda codes, scales, kv_bit, pos, k, v: dict(slab=codes, pos=pos, n=_n(k)),
    "attention_blhc": lambda q, k, v, scale: dict(seq=_n(k), n=_n(q)),
    "attention_blhc_kvcodes": lambda q, codes, scales, kv_bit, n_packed, k, v, scale: dict(slab=codes, n_packed=n_packed, n=_n(k)),
    "scaled_dot_product_attention": lambda q, k, v, **kw: dict(seq=int(k.shape[2]), n=int(q.shape[2])),   # [B, H, L, c]
    "linear_fp4_qkv_to_cache": lambda a, sa, w, sw, bias, cache_kv, pos, seq, *r, **kw: dict(slab=cache_kv, pos=pos, seq=seq),
    "linear_fp6_qkv_to_cache": lambda a, sa, w, sw, bias, cache_kv, pos, seq, *r, **kw: dict(slab=cache_kv, pos=pos, seq=seq),
}
RECORDED = {
    "ops": ("kv_cache_step", "kv_cache_step_qk_norm", "kv_pack", "attention_blhc", "attention_blhc_kvcodes", "gate_residual"),
    "gemm": ("quantize_mx", "quantize_fp6", "linear_fp4", "linear_fp6", "linear_fp4_qkv_to_cache", "linear_fp6_qkv_to_cache",
             "linear_fp4_gelu_dual"),
    "rotation": ("adaln_rotate_quant", "adaln_rotate_quant_token", "adaln_rotate_quant_mx", "resid_adaln_rotate_quant",
                 "resid_adaln_rotate_quant_token", "resid_adaln_rotate_quant_mx"),
    "quant_utils": ("fp_quant_e2_per_group_cuda", "fp6_quant_e2m3_per_token_cuda", "fp_quant_e1m2_neg_e2m1_pos_per_group_cuda",
                    "fp6_quant_int_neg_e2m3_pos_per_token_cuda", "gelu_fp_quant_e1m2_neg_e2m1_pos_per_group_cuda",
                    "gelu_fp6_quant_int_neg_e2m3_pos_per_token_cuda"),
}


class _Recorder:
    """Forwarding wrappers around the functions above; a call made from inside another recorded call is that call's own business and
    is not listed.  `owners`: data_ptr of a slab -> "cache<b>" / "staging"."""

    def __init__(self):
        self.trace, self.owners, self.depth = [], {}, 0

    def wrap(self, name, inner):
        @functools.wraps(inner)
        def forward(*args, **kwargs):
            if self.depth == 0:
                entry = {"name": name}
                if name in FACING:
                    entry.update(FACING[name](*args, **kwargs))
                    if "slab" in entry:
                        entry["slab"] = self.owners.get(entry["slab"].data_ptr(), "neither the block's cache nor the staging slab")
                if name.endswith("_token"):       # the W6A6 producers: fake-quantized values (path F) or the FP6 GEMM's operands (path Q)
                    entry["emit"] = kwargs.get("emit", "values")
                self.trace.append(entry)
            self.depth += 1
            try:
                return inner(*args, **kwargs)
            finally:
                self.depth -= 1
        return forward

    def install(self, patch):
        import torch.nn.functional as Fn
        from fpqvar_amd import gemm, ops, quant_utils, rotation
        mods = {"ops": ops, "gemm": gemm, "rotation": rotation, "quant_utils": quant_utils}
        for mod, names in RECORDED.items():
            for name in names:
                patch.setattr(mods[mod], name, self.wrap(name, getattr(mods[mod], name)))
        patch.setattr(Fn, "scaled_dot_product_attention", self.wrap("scaled_dot_product_attention", Fn.scaled_dot_product_attention))


def _cache_state(cache):
    """the filled part of a block's cache, as CPU tensors"""
    if hasattr(cache, "codes"):
        return [cache.codes[:, :, :cache.len].cpu(), cache.scales[:, :, :cache.len].cpu()]
    return [cache.kv[:, :, :cache.len].cpu()]


@functools.lru_cache(maxsize=None)
def _run(case):
    """The three steps of one case, run once: (step outputs, per-block cache state after the last step, per-step traces), on the CPU."""
    from fpqvar_amd import var_block
    path, config, storage, norm, fuse, split, sdpa = case
    gb = var_block.GenerationBatch(MODEL, config, depth=DEPTH, batch_rows=ROWS, device=torch.device("cuda:0"), sdpa_in_f=sdpa,
                                   qkv_to_cache=split, attn_l2_norm=norm != "off", qk_norm="torch" if norm == "torch" else "fused",
                                   kv_storage=storage, fuse_residual=fuse)
    caches = gb.new_caches(path)
    rec = _Recorder()
    for b, c in enumerate(caches):
        rec.owners[(c.codes if hasattr(c, "codes") else c.kv).data_ptr()] = f"cache{b}"
        if getattr(c, "staging", None) is not None:
            rec.owners[c.staging.data_ptr()] = "staging"
    outs, traces = [], []
    with pytest.MonkeyPatch.context() as patch:
        xs = [gb.new_input(pn) for pn in STEPS]
        rec.install(patch)
        for x in xs:
            rec.trace = []
            outs.append(gb.step(path, caches, x).cpu())
            traces.append(rec.trace)
    torch.cuda.synchronize()
    assert [c.len for c in caches] == [sum(pn * pn for pn in STEPS)] * DEPTH
    return outs, [_cache_state(c) for c in caches], traces


def digest(case) -> str:
    """one sha256 over every step output and every block's cache contents of a case (tools compare two trees with it)"""
    outs, states, _ = _run(case)
    h = hashlib.sha256()
    for t in itertools.chain(outs, *states):
        h.update(str((t.dtype, tuple(t.shape))).encode())
        h.update(t.contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


# ---- the expected trace, from the case's parameters ------------------------------------------------------------------------------
def _expected(case, b, length, prev, L):
    """block b of a step of L tokens on a cache that holds `length` tokens, the last step's from `prev` on"""
    path, config, storage, norm, fuse, split, sdpa = case
    w6 = config == "w6a6"
    own = f"cache{b}"

    def producer(pending):
        head = "resid_" if pending else ""
        if w6:
            return {"name": head + "adaln_rotate_quant_token", "emit": "values" if path == "F" else "fp6"}
        return {"name": head + ("adaln_rotate_quant" if path == "F" else "adaln_rotate_quant_mx")}

    linear = {"name": "linear_fp6" if w6 else "linear_fp4"}
    quant = {"name": "quantize_fp6" if w6 else "quantize_mx"}
    if sdpa:
        attention = {"name": "scaled_dot_product_attention", "seq": length + L, "n": L}
    else:
        attention = {"name": "attention_blhc", "seq": length + L, "n": L}
    packed = [{"name": "attention_blhc_kvcodes", "slab": own, "n_packed": length, "n": L}, {"name": "kv_pack", "slab": own, "pos": length, "n": L}]
    kv_step = {"slab": own, "quant_start": prev, "quant_stop": length, "new_start": length}

    seq = [producer(fuse and b > 0)]
    if path == "Q" and split and norm != "torch":          # k / v (normalized in the epilogue with the fused norm) written by the GEMM
        name = "linear_fp6_qkv_to_cache" if w6 else "linear_fp4_qkv_to_cache"
        if storage == "codes":
            seq += [{"name": name, "slab": "staging", "pos": 0, "seq": L}, *packed]
        else:
            seq += [{"name": name, "slab": own, "pos": length, "seq": L}]
            seq += [{"name": "kv_cache_step", **kv_step, "n": 0}] if length > prev else []
            seq += [attention]
    else:
        seq += [linear] if path == "Q" else []
        if storage == "codes":
            if norm == "fused":
                seq += [{"name": "kv_cache_step_qk_norm", "slab": "staging", "quant_start": 0, "quant_stop": 0, "new_start": 0, "n": L}]
            seq += packed
        else:
            seq += [{"name": "kv_cache_step_qk_norm" if norm == "fused" else "kv_cache_step", **kv_step, "n": L}, attention]
    last = b + 1 == DEPTH
    if path == "F":
        seq += [{"name": "fp6_quant_e2m3_per_token_cuda" if w6 else "fp_quant_e2_per_group_cuda"}]                 # proj's input
        seq += [producer(True)] if fuse else [{"name": "gate_residual"}, producer(False)]                             # proj's tail, fc1's input
        seq += [{"name": "gelu_fp6_quant_int_neg_e2m3_pos_per_token_cuda" if w6 else "gelu_fp_quant_e1m2_neg_e2m1_pos_per_group_cuda"}]
    else:
        seq += [quant, linear, producer(False)]                                                                        # proj with its tail, fc1's input
        seq += [linear, {"name": "gelu_fp6_quant_int_neg_e2m3_pos_per_token_cuda"}] if w6 else [{"name": "linear_fp4_gelu_dual"}]
    seq += [] if (fuse and not last) else [{"name": "gate_residual"}]                                               # fc2's tail
    return seq


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_call_trace(case):
    _, _, traces = _run(case)
    length = prev = 0
    for pn, trace in zip(STEPS, traces):
        L = pn * pn
        want = [_expected(case, b, length, prev, L) for b in range(DEPTH)]
        at = 0
        for b, block in enumerate(want):
            got = trace[at:at + len(block)]
            assert got == block, f"step of {L} tokens, block {b}:\n got  {got}\n want {block}"
            at += len(block)
        assert trace[at:] == [], f"step of {L} tokens: calls after the last block: {trace[at:]}"
        prev, length = length, length + L


# ---- bit equality across options -------------------------------------------------------------------------------------------------
def _same_outputs(a, b, what):
    for i, (x, y) in enumerate(zip(_run(a)[0], _run(b)[0])):
        assert_bits_equal(x, y, f"{what}: output of step {i}")


def _replace(case, **kw):
    d = dict(zip(("path", "config", "storage", "norm", "fuse", "split", "sdpa"), case))
    d.update(kw)
    return tuple(d.values())


@pytest.mark.parametrize("case", [c for c in CASES if c[2] == "fp16" and not c[6]], ids=case_id)
def test_kv_storage_changes_no_bit(case):
    _same_outputs(case, _replace(case, storage="codes"), "fp16 cache against codes")


@pytest.mark.parametrize("case", [c for c in CASES if not c[4]], ids=case_id)
def test_fuse_residual_changes_no_bit(case):
    _same_outputs(case, _replace(case, fuse=True), "fuse_residual off against on")


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == "Q" and c[3] == "off" and c[5]], ids=case_id)
def test_qkv_to_cache_changes_no_bit(case):
    other = _replace(case, split=False)
    _same_outputs(case, other, "split output against copy-in")
    for b, (sa, sb) in enumerate(zip(_run(case)[1], _run(other)[1])):
        for x, y in zip(sa, sb):
            if x.dtype == torch.uint8:
                assert torch.equal(x, y), f"split output against copy-in: codes of block {b}"
            else:
                assert_bits_equal(x, y, f"split output against copy-in: cache of block {b}")
