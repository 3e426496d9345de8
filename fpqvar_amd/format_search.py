"""Per-layer format search inner loop (reference: search/search_fp6_format.py:584-608,
827-846 and its FP4 twin search/search_fp4_format.py): for every (weight format,
activation format) pair accumulate  mean((x_j W^T - q_a(x_j) q_w(W)^T)^2)  over the
calibration activations x_j and keep the argmin.  The quantizers are this package's
fused kernels; the two GEMMs are plain library calls.  Blocks are independent, so the
search shards by block over the ranks of a process group and ends with one tiny
all-gather of (loss, w_fmt, a_fmt) per block.
"""
from __future__ import annotations

from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from . import ops
from . import quant_utils as qu

# the reference's candidate sets
FP6_FORMATS = ("fp6_e2m3", "fp6_e3m2")                 # per-token quantizers (search_fp6_format.py:513-554)
FP4_FORMATS = ("fp_e1", "fp_e2", "fp_e3")              # per-group-128 quantizers (search_fp4_format.py:484-553)


def quantizer(fmt: str) -> Callable[[torch.Tensor], torch.Tensor]:
    table = {
        "fp6_e2m3": lambda t: qu.fp6_quant_e2m3_per_token_cuda(t, 6),
        "fp6_e3m2": lambda t: qu.fp6_quant_e3m2_per_token_cuda(t, 6),
        "fp_e1": lambda t: qu.fp_quant_e1_per_group_cuda(t, 4, 128),
        "fp_e2": lambda t: qu.fp_quant_e2_per_group_cuda(t, 4, 128),
        "fp_e3": lambda t: qu.fp_quant_e3_per_group_cuda(t, 4, 128),
    }
    return table[fmt]


def sample_row_weights(rows_per_sample: Sequence[int], outs: int, device) -> torch.Tensor:
    """float32 [sum rows]: 1 / (rows_j * outs) repeated rows_j times - the weight of a row of sample j, so that
    sum_j mean_j(e^2) = sum over rows of (the row's squared error) * (the row's weight).  Built on the host and copied once:
    the same bits as the vector the batched form of search_layer builds inline on the device."""
    rows = [int(r) for r in rows_per_sample]
    per_sample = torch.tensor([1.0 / (r * outs) for r in rows], dtype=torch.float32)
    return torch.repeat_interleave(per_sample, torch.tensor(rows, dtype=torch.int64)).to(device)


def pick_winner(losses_2d_host, formats: Sequence[str]) -> Tuple[str, str]:
    """(weight format, activation format) of the smallest entry of losses[w index][a index] (a host tensor or nested
    sequences); ties go to the smaller weight index, then the smaller activation index."""
    nf = len(formats)
    keys = [(i, j) for i in range(nf) for j in range(nf)]
    i, j = min(keys, key=lambda k: (float(losses_2d_host[k[0]][k[1]]), k[0], k[1]))
    return formats[i], formats[j]


_ROW_WEIGHTS: Dict[tuple, torch.Tensor] = {}


def _row_weights_on_device(rows: Sequence[int], outs: int, device) -> torch.Tensor:
    """sample_row_weights on the device without a synchronising copy: the blocks of a search share one calibration set, so
    the vector is kept per (sample sizes, outs, device); a new one travels from pinned memory, asynchronously."""
    key = (tuple(rows), outs, str(device))
    t = _ROW_WEIGHTS.get(key)
    if t is None:
        if len(_ROW_WEIGHTS) >= 8:
            _ROW_WEIGHTS.clear()
        t = _ROW_WEIGHTS[key] = sample_row_weights(rows, outs, "cpu").pin_memory().to(device, non_blocking=True)
    return t


def _search_layer_fused(xs: Sequence[torch.Tensor], w: torch.Tensor, formats: Sequence[str], quant: Callable[[str], Callable],
                        losses_out: torch.Tensor) -> None:
    """The batched arithmetic with the loss in one fused pass per weight format: the activation formats' quantized rows
    stacked along the row axis, ONE GEMM per weight format, the product kept in w's dtype, and one
    ops.sqerr_rows_weighted call (the reference product read once for all activation formats) into row i of losses_out."""
    nf = len(formats)
    c, outs = w.shape[-1], w.shape[0]
    rows = [x.numel() // c for x in xs]
    x_all = torch.cat([x.reshape(-1, c) for x in xs])
    w_row = _row_weights_on_device(rows, outs, w.device)
    ref = x_all.to(w.dtype) @ w.t()
    xq = torch.cat([quant(af)(x_all).to(w.dtype) for af in formats])                 # [nf * rows, C]: one launch per format
    for i, wf in enumerate(formats):
        wq = quant(wf)(w).to(w.dtype)
        y = (xq @ wq.t()).view(nf, x_all.shape[0], outs)
        ops.sqerr_rows_weighted(ref, y, w_row, out=losses_out[i])


def _mc_operand(fmt: str, t: torch.Tensor, weight: bool):
    """A search format's matrix-core operand of t [rows, C] - the codes and scales the deployed Linears multiply:
      fp_e2                  quantize_mx: E2M1 nibbles, a scale per group of 128
      fp_e1 / fp_e3          quantize_g6: dense 6-bit codes of the E1M2 / E3M0 levels, a scale per group
      fp6_e2m3 / fp6_e3m2    quantize_fp6(table=): dense 6-bit codes, a scale per token / per output channel
    Every operand is quantized in its own dtype, as the search's fake-quantizers see it, so both forms of the search judge the
    same codes - except an fp_e1 / fp_e3 WEIGHT, which is quantized from its fp32 copy as FP4Linear.from_float(weight_fp_type=)
    builds it: the W6 GEMM takes fp32 group scales only.  For an fp32 weight that is the same thing; for an fp16 weight the
    scales are not rounded to fp16, a few level decisions near a midpoint fall the other way, and at a small layer that alone
    moves a loss by up to 1.5e-3 relative (tests/test_gpu_format_search_mc.py; 5e-5 at a d30 mat_qkv layer)."""
    from . import gemm
    if fmt == "fp_e2":
        return gemm.quantize_mx(t)
    if fmt in ("fp_e1", "fp_e3"):
        return gemm.quantize_g6(t.float() if weight else t, fmt)
    return gemm.quantize_fp6(t, table=fmt)


def _mc_loss(wf: str, af: str, w_op, a_op, ref: torch.Tensor, w_row: torch.Tensor, out: torch.Tensor) -> None:
    """One GEMM-with-loss call of the pair's family (gemm.linear_*_sqerr) into the one-element view `out`"""
    from . import gemm
    if wf in FP6_FORMATS:                                   # (the pair is FP6 x FP6: _search_layer_mc has checked it)
        gemm.linear_fp6_sqerr(*a_op, *w_op, ref, w_row, out=out, a_table=af, w_table=wf)
    elif wf != "fp_e2":
        gemm.linear_w6_sqerr(*a_op, af, *w_op, wf, ref, w_row, out=out)
    elif af != "fp_e2":
        gemm.linear_a6w4_sqerr(*a_op, af, *w_op, ref, w_row, out=out)
    else:
        gemm.linear_fp4_sqerr(*a_op, *w_op, ref, w_row, out=out)


def _search_layer_mc(xs: Sequence[torch.Tensor], w: torch.Tensor, formats: Sequence[str], losses_out: torch.Tensor) -> None:
    """The fused form with every candidate product on the matrix cores and its loss in that GEMM's epilogue: activations
    quantized to operand codes once per activation format, the weight once per weight format, the reference product one torch
    GEMM in w's dtype as in _search_layer_fused, then ONE call per pair into losses_out[i, j] - no candidate product is written
    to memory, nothing is read back."""
    per_group = all(f in FP4_FORMATS for f in formats)
    if not per_group and not all(f in FP6_FORMATS for f in formats):
        raise RuntimeError(f"search_layer(matrix_cores=True) takes the FP4 formats {FP4_FORMATS} or the FP6 formats {FP6_FORMATS}, "
                           f"not a mix and nothing else, got {tuple(formats)}")
    if any(x.dtype != torch.float16 for x in xs):
        raise RuntimeError("search_layer(matrix_cores=True) requires float16 activations (the GEMMs' activation scales are float16)")
    c, outs = w.shape[-1], w.shape[0]
    if c % 128 != 0:
        raise RuntimeError(f"search_layer(matrix_cores=True) requires K % 128 == 0 (the matrix instruction's K step), got K = {c}")
    if outs % 8 != 0:
        raise RuntimeError(f"search_layer(matrix_cores=True) requires outs % 8 == 0, got {outs}")
    rows = [x.numel() // c for x in xs]
    x_all = torch.cat([x.reshape(-1, c) for x in xs])
    w_row = _row_weights_on_device(rows, outs, w.device)
    ref = x_all.to(w.dtype) @ w.t()
    a_ops = [_mc_operand(af, x_all, False) for af in formats]
    for i, wf in enumerate(formats):
        w_op = _mc_operand(wf, w, True)
        for j, af in enumerate(formats):
            _mc_loss(wf, af, w_op, a_ops[j], ref, w_row, losses_out[i, j])


@torch.no_grad()
def search_layer(xs: Sequence[torch.Tensor], w: torch.Tensor, formats: Sequence[str] = FP6_FORMATS,
                 quant: Callable[[str], Callable] = quantizer, batched: Optional[bool] = None, fused: bool = False,
                 losses_out: Optional[torch.Tensor] = None,
                 matrix_cores: bool = False) -> Optional[Tuple[str, str, Dict[Tuple[str, str], float]]]:
    """(best weight format, best activation format, {(w_fmt, a_fmt): summed MSE}).

    The reference walks the calibration samples one by one for every (w_fmt, a_fmt) pair: per sample one quantizer call
    (~11 torch ops + the scan kernel), two GEMMs, an MSE and a host sync (`.item()`), search_fp6_format.py:589-608.
    batched=True (default) does the same arithmetic on ALL samples of the layer at once: every quantizer here works row
    by row (per token) or group by group, so the samples are concatenated along their rows - ONE quantizer launch per
    activation format for the whole calibration set (and one per weight format), ONE GEMM per pair, the per-sample
    means as a weighted row reduction, all `len(formats)^2` losses kept on the device and read back with ONE copy.
    batched=False is the sample-by-sample loop (same quantizers), kept for comparison and for tests.

    Precondition of the batched form: the quantizer must be ROW-LOCAL (per token, or per group inside a row) - a
    per-tensor quantizer sees a different tensor once the samples are concatenated.  The built-in `quantizer` table is;
    an injected `quant` is not assumed to be: batched=None (default) means "batched for the built-in quantizers, the
    loop for anything injected", and a caller who knows his quantizer to be row-local passes batched=True.
    Both forms quantize x in ITS dtype (the reference calls the quantizer on the dumped activation as it is), cast to
    the weight's dtype for the GEMM, and subtract in float32.

    fused=True (batched only, CUDA tensors, an fp16 or fp32 weight, at most four formats): the same operands, but the
    products stay in w's dtype and the five elementwise passes per pair become one ops.sqerr_rows_weighted pass per WEIGHT
    format (fpq_sqerr_rows_weighted: fp32 difference, square and sums in a fixed order).  With losses_out (a device
    [nf, nf] float32 tensor) the losses are left there, nothing is read back and None is returned; without it, one `.cpu()`
    and the same triple as the other forms.  The default (fused=False) is unchanged.

    matrix_cores=True (with fused=True; the built-in formats only - an injected `quant` is refused; float16 activations, K a
    multiple of 128, outs a multiple of 8): every candidate product runs on the matrix-core GEMM the deployed model runs for that
    pair - fp_e2 x fp_e2 on the FP4 GEMM, an fp_e1 / fp_e3 activation against fp_e2 weights on the A6W4 GEMM, fp_e1 / fp_e3
    weights on the W6 GEMM, the FP6 pairs on the row-scaled FP6 GEMM - with the loss in that GEMM's epilogue
    (gemm.linear_*_sqerr): operands quantized once per format, one call per pair, no candidate product written to memory.  The
    search then judges a pair by the product the quantized model computes (exact products of the levels, fp32 accumulation, one
    rounding to fp16) instead of an fp16 GEMM of fake-quantized tensors; the two agree to the search's tolerance between
    evaluation orders, not bit for bit.  Off by default."""
    nf = len(formats)
    if batched is None:
        batched = quant is quantizer
    if matrix_cores:
        if not fused:
            raise RuntimeError("search_layer: matrix_cores=True is a variant of the fused form (fused=True)")
        if quant is not quantizer:
            raise RuntimeError("search_layer(matrix_cores=True) runs the built-in formats' own operand quantizers: an injected `quant` is refused")
    if fused or losses_out is not None:
        if not fused:
            raise RuntimeError("search_layer: losses_out is an argument of the fused form (fused=True)")
        if not batched:
            raise RuntimeError("search_layer(fused=True) requires the batched form (batched=True, a row-local quantizer)")
        if not w.is_cuda or not all(x.is_cuda for x in xs):
            raise RuntimeError("search_layer(fused=True) requires CUDA tensors (the fused loss is a GPU kernel, there is no CPU path)")
        if w.dtype not in (torch.float16, torch.float32):
            raise RuntimeError(f"search_layer(fused=True) requires a float16 or float32 weight, got {w.dtype}")
        if not 1 <= nf <= 4:
            raise RuntimeError(f"search_layer(fused=True) takes 1 to 4 formats (the planes of one fused pass), got {nf}")
        out = losses_out if losses_out is not None else torch.empty(nf, nf, dtype=torch.float32, device=w.device)
        if out.shape != (nf, nf) or out.dtype != torch.float32 or out.device != w.device or not out.is_contiguous():
            raise RuntimeError(f"search_layer(fused=True): losses_out must be a contiguous float32 [{nf}, {nf}] tensor on the weight's device")
        if matrix_cores:
            _search_layer_mc(xs, w, formats, out)
        else:
            _search_layer_fused(xs, w, formats, quant, out)
        if losses_out is not None:
            return None
        host = out.cpu()                                                               # the layer's one synchronisation
        losses = {(wf, af): float(host[i, j]) for i, wf in enumerate(formats) for j, af in enumerate(formats)}
    elif not batched:
        losses: Dict[Tuple[str, str], float] = {}
        refs = [x.to(w.dtype) @ w.t() for x in xs]
        for wf in formats:
            wq = quant(wf)(w).to(w.dtype)
            for af in formats:
                qa = quant(af)
                total = torch.zeros((), dtype=torch.float32, device=w.device)
                for x, ref in zip(xs, refs):
                    y = qa(x).to(w.dtype) @ wq.t()
                    total += torch.mean((ref.float() - y.float()) ** 2)
                losses[(wf, af)] = float(total)
    else:
        c = w.shape[-1]
        rows = [x.numel() // c for x in xs]
        x_all = torch.cat([x.reshape(-1, c) for x in xs])                             # [sum rows, C], the samples' dtype
        # sum_j mean_j((y - y_q)^2) = sum over rows of (row's squared error) / (rows_j * out): one weight per row
        w_row = torch.repeat_interleave(torch.tensor([1.0 / (r * w.shape[0]) for r in rows], dtype=torch.float32, device=w.device),
                                        torch.tensor(rows, device=w.device))
        ref = (x_all.to(w.dtype) @ w.t()).float()
        xq = {af: quant(af)(x_all).to(w.dtype) for af in formats}                     # one launch per activation format
        out = torch.empty(nf, nf, dtype=torch.float32, device=w.device)
        for i, wf in enumerate(formats):
            wq = quant(wf)(w).to(w.dtype)
            for j, af in enumerate(formats):
                d = ref - (xq[af] @ wq.t()).float()
                out[i, j] = torch.dot((d * d).sum(dim=1), w_row)
        host = out.cpu()                                                               # the layer's one synchronisation
        losses = {(wf, af): float(host[i, j]) for i, wf in enumerate(formats) for j, af in enumerate(formats)}
    wf, af = pick_winner([[losses[(a, b)] for b in formats] for a in formats], formats)
    return wf, af, losses


@torch.no_grad()
def search_layers_fused(layers: Iterable[Tuple[Sequence[torch.Tensor], torch.Tensor]], formats: Sequence[str] = FP6_FORMATS,
                        quant: Callable[[str], Callable] = quantizer, matrix_cores: bool = False) -> torch.Tensor:
    """search_layer(fused=True) over an iterable of (xs, w): float32 [L, nf, nf] on the device, nothing read back and no
    synchronisation inside - the caller's one `.cpu()` serves every layer.  matrix_cores: as in search_layer."""
    nf = len(formats)
    tables = []
    for xs, w in layers:
        t = torch.empty(nf, nf, dtype=torch.float32, device=w.device)
        search_layer(xs, w, formats, quant, batched=True, fused=True, losses_out=t, matrix_cores=matrix_cores)
        tables.append(t)
    if not tables:
        return torch.empty(0, nf, nf, dtype=torch.float32)
    return torch.stack(tables)


def _gather_triples(buf: torch.Tensor, n_blocks: int, formats: Sequence[str], group, world: int) -> List[Tuple[str, str, float]]:
    """This rank's (loss, w index, a index) rows -> every block's (w_fmt, a_fmt, loss) on every rank: one all-gather."""
    if world == 1:
        gathered = [buf]
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else buf.device
        send = buf.to(dev)
        gathered = [torch.empty_like(send) for _ in range(world)]
        dist.all_gather(gathered, send, group=group)
        gathered = [g.cpu() for g in gathered]
    out: List[Optional[Tuple[str, str, float]]] = [None] * n_blocks
    for r in range(world):
        for slot, b in enumerate(range(r, n_blocks, world)):
            loss, wi, ai = gathered[r][slot].tolist()
            out[b] = (formats[int(wi)], formats[int(ai)], loss)
    return out  # type: ignore[return-value]


def search_blocks_sharded(n_blocks: int, evaluate: Callable[[int], Tuple[str, str, float]],
                          formats: Sequence[str] = FP6_FORMATS, group=None) -> List[Tuple[str, str, float]]:
    """Block b is evaluated on rank b % world; every rank gets all results.
    `evaluate(b)` returns (w_fmt, a_fmt, loss).  The collective is one all-gather of
    n_blocks x (loss, w index, a index) float32 triples."""
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    per_rank = (n_blocks + world - 1) // world
    buf = torch.full((per_rank, 3), -1.0, dtype=torch.float32)
    for slot, b in enumerate(range(rank, n_blocks, world)):
        wf, af, loss = evaluate(b)
        buf[slot] = torch.tensor([loss, formats.index(wf), formats.index(af)], dtype=torch.float32)
    return _gather_triples(buf, n_blocks, formats, group, world)


def search_blocks_sharded_fused(n_blocks: int, layer_of: Callable[[int], Tuple[Sequence[torch.Tensor], torch.Tensor]],
                                formats: Sequence[str] = FP6_FORMATS, group=None, matrix_cores: bool = False) -> List[Tuple[str, str, float]]:
    """search_blocks_sharded on the fused form: `layer_of(b)` returns block b's (xs, w); this rank's blocks (b % world ==
    rank) go through search_layers_fused, their losses are read back ONCE, the winners are picked on the host, and the
    same all-gather of triples follows.  matrix_cores: as in search_layer."""
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    per_rank = (n_blocks + world - 1) // world
    buf = torch.full((per_rank, 3), -1.0, dtype=torch.float32)
    host = search_layers_fused((layer_of(b) for b in range(rank, n_blocks, world)), formats, matrix_cores=matrix_cores).cpu()
    for slot in range(host.shape[0]):
        wf, af = pick_winner(host[slot], formats)
        i, j = formats.index(wf), formats.index(af)
        buf[slot] = torch.tensor([float(host[slot, i, j]), i, j], dtype=torch.float32)
    return _gather_triples(buf, n_blocks, formats, group, world)
