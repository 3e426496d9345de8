"""Which kernel each producer call launches: a walk over the host dispatch of fpq_kernels.hip, fpq_rotate.hip and fpq_adaln.hip.

Bit-exact parity cannot see the dispatch (two equally correct kernels give the same bits), so a change of it is checked by
tracing: the same flat list of calls is run under the profiler on two builds of the library, and the two traces must be
the same sequence of (kernel, grid, workgroup, LDS).

    rocprofv3 --kernel-trace --stats -d DIR_A -- python tools/launch_walk.py --lib BEFORE.so
    rocprofv3 --kernel-trace --stats -d DIR_B -- python tools/launch_walk.py --lib AFTER.so
    python tools/launch_walk.py --compare DIR_A DIR_B [--kernels-of AFTER.so]      (no GPU needed)

Every row is (label, entry point, arguments, options): the arguments are sizes and ids, the pointers are zero-filled device
buffers large enough for the row (checked before the call); the options go through _lib.option (the library reads its option
table at every call, so no row needs a process of its own).  One label is printed per row.  --compare prints "identical" or
the first differing launch, and with --kernels-of the kernels of the three producer units that the walk never launched."""
import argparse
import csv
import ctypes
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, F32, F64 = 0, 1, 2
E2M1, E1M2, E3M0, E2M3, E3M2, E1M2_NEG, E2M1_POS, INT_NEG, E2M3_POS, E2M1_NEG = range(10)
SYM = {"e2m1": E2M1, "e1m2": E1M2, "e3m0": E3M0, "e2m3": E2M3, "e3m2": E3M2}
MIB = 1 << 20
BIG, SMALL = 320 * MIB, 64 * MIB      # x / out; every other operand


def rows_table():
    """[(label, entry, kwargs, {option: value})].  kwargs: sizes and ids by the names of call(); pointer arguments are named
    by call()."""
    R = []

    def add(label, entry, opts=None, **kw):
        R.append((label, entry, kw, opts or {}))

    # ---- element scans
    for dt in (F32, F64):
        add(f"nearest dtype={dt}", "fpq_quant_nearest", n=5000, k=8, dtype=dt)
    for dt in (F16, F32):
        add(f"nearest_argmin dtype={dt}", "fpq_quant_nearest_argmin", n=5000, k=8, dtype=dt)
    add("nearest_builtin", "fpq_quant_nearest_builtin", n=5000, table_id=E2M3)
    # ---- fpq_quant_rows, fp16 -> fp16: launch_fast16 / launch_fast16_block
    for name, t in SYM.items():
        for cols in (8, 16, 32, 64, 128, 256, 512, 24, 1024, 1920, 2304, 4096, 7680, 10240, 16384, 16392, 100):
            add(f"rows16 {name} c={cols}", "fpq_quant_rows", rows=40, cols=cols, table_id=t, in_dtype=F16, out_dtype=F16)
    for opt in ("FPQ_NO_HW4", "FPQ_NO_HW6", "FPQ_NO_WAVE_ROWS"):
        for name in ("e2m1", "e2m3", "e3m2"):
            for cols in (64, 128, 1024, 1920, 2304):
                add(f"rows16 {name} c={cols} {opt}", "fpq_quant_rows", {opt: 1}, rows=40, cols=cols, table_id=SYM[name], in_dtype=F16, out_dtype=F16)
    for rows in (64, 65544):     # the wave forms' cap of 16384 workgroups (four rows each)
        add(f"rows16 e2m1 c=1024 r={rows}", "fpq_quant_rows", rows=rows, cols=1024, table_id=E2M1, in_dtype=F16, out_dtype=F16)
    for rows in (64, 524352):    # tables of >= 1024 buckets on the sub-wavefront forms: at most 16384 workgroups
        add(f"rows16 e2m3 c=128 r={rows} FPQ_NO_HW6", "fpq_quant_rows", {"FPQ_NO_HW6": 1}, rows=rows, cols=128, table_id=E2M3, in_dtype=F16, out_dtype=F16)
    for rpb in (1, 3):
        add(f"rows16 e2m3 c=7680 FPQ_BIGTAB_RPB={rpb}", "fpq_quant_rows", {"FPQ_BIGTAB_RPB": rpb}, rows=40, cols=7680, table_id=E2M3, in_dtype=F16, out_dtype=F16)
    # ---- fpq_quant_rows, the other dtypes: fast32 / rows32 / launch_rows
    for od in (F16, F32):
        for cols in (4, 8, 16, 32, 64, 128, 256, 384, 512, 1024, 2048, 3072, 4096, 6144, 8192, 10240, 16384, 100, 102):
            add(f"rows32 c={cols} out={od}", "fpq_quant_rows", rows=24, cols=cols, table_id=E2M1, in_dtype=F32, out_dtype=od)
        for cols in (128, 512, 2048):
            add(f"rows32 c={cols} out={od} FPQ_NO_FAST32", "fpq_quant_rows", {"FPQ_NO_FAST32": 1}, rows=24, cols=cols, table_id=E2M1, in_dtype=F32, out_dtype=od)
    for cols in (8, 16, 32, 64, 128, 256, 512, 1024, 8192, 100):
        add(f"rows16->32 c={cols}", "fpq_quant_rows", rows=24, cols=cols, table_id=E3M0, in_dtype=F16, out_dtype=F32)
    add("rows16 misaligned", "fpq_quant_rows", rows=24, cols=128, table_id=E2M1, in_dtype=F16, out_dtype=F16, x_off=2)
    # ---- several tensors in one call
    for cols in (8, 16, 32, 64, 128, 256, 512, 1024):
        add(f"multi c={cols}", "fpq_quant_rows_multi", seg_rows=(24, 40, 8), cols=cols, table_id=E2M1, in_dtype=F16, out_dtype=F16)
    add("multi fp32", "fpq_quant_rows_multi", seg_rows=(24, 40), cols=128, table_id=E2M1, in_dtype=F32, out_dtype=F16)
    for od in (F16, F32):
        add(f"segments out={od}", "fpq_quant_rows_segments", seg_rows=(24, 40, 8), cols=128, table_id=E2M1, in_dtype=F32, out_dtype=od)
    # ---- the KV cache
    for group in (8, 16, 32, 64, 128, 256, 512):
        add(f"kv_step g={group}", "fpq_kv_cache_step", group=group, table_id=E2M3)
    for group in (64, 128):
        add(f"kv_step_qknorm g={group}", "fpq_kv_cache_step_qknorm", group=group, table_id=E2M3)
    for bit in (6, 4):
        add(f"kv_pack {bit}", "fpq_kv_pack", kv_bit=bit)
    # ---- argmin semantics, negative-reversed rows: launch_rows / launch_negrev
    for dt in (F16, F32):
        for cols in (4, 8, 16, 32, 64, 128, 256, 512, 1024, 8192, 100):
            add(f"rows_argmin in={dt} c={cols}", "fpq_quant_rows_argmin", rows=24, cols=cols, table_id=E2M1, in_dtype=dt, clamp3=1)
            add(f"dual_argmin in={dt} c={cols}", "fpq_quant_rows_dual_argmin", rows=24, cols=cols, neg=E1M2_NEG, pos=E2M1_POS, in_dtype=dt)
            add(f"neg_reverse dt={dt} c={cols}", "fpq_quant_rows_neg_reverse", rows=24, cols=cols, table_id=E2M1, dtype=dt)
    # ---- dual format
    for neg, pos in ((E1M2_NEG, E2M1_POS), (E2M1_NEG, E2M3_POS), (INT_NEG, E2M3_POS)):
        for cols in (8, 16, 32, 64, 128, 256, 512, 24, 1024, 1920, 2304, 4096, 7680, 10240, 16384, 100):
            add(f"dual {neg}/{pos} c={cols}", "fpq_quant_rows_dual", rows=40, cols=cols, neg=neg, pos=pos, in_dtype=F16, out_dtype=F16)
        add(f"dual {neg}/{pos} c=128 flag", "fpq_quant_rows_dual", rows=40, cols=128, neg=neg, pos=pos, in_dtype=F16, out_dtype=F16, flag=True)
        add(f"dual {neg}/{pos} c=128 clip", "fpq_quant_rows_dual", rows=40, cols=128, neg=neg, pos=pos, in_dtype=F16, out_dtype=F16, clip=True)
        add(f"dual {neg}/{pos} c=256 clip", "fpq_quant_rows_dual", rows=40, cols=256, neg=neg, pos=pos, in_dtype=F16, out_dtype=F16, clip=True)
        add(f"dual {neg}/{pos} c=1920 FPQ_NO_WAVE_ROWS", "fpq_quant_rows_dual", {"FPQ_NO_WAVE_ROWS": 1}, rows=40, cols=1920, neg=neg, pos=pos, in_dtype=F16, out_dtype=F16)
        for cols in (128, 1024, 1920, 4096, 7680, 10240, 16384):
            add(f"gelu_dual {neg}/{pos} c={cols}", "fpq_gelu_quant_rows_dual", rows=40, cols=cols, neg=neg, pos=pos, flag=cols == 128)
    for cap in (4096, 8):
        add(f"dual int_neg/e2m3_pos c=128 FPQ_BIGTAB_CAP={cap}", "fpq_quant_rows_dual", {"FPQ_BIGTAB_CAP": cap}, rows=4096, cols=128, neg=INT_NEG, pos=E2M3_POS, in_dtype=F16, out_dtype=F16)
        add(f"gelu_dual int_neg/e2m3_pos c=128 FPQ_BIGTAB_CAP={cap}", "fpq_gelu_quant_rows_dual", {"FPQ_BIGTAB_CAP": cap}, rows=4096, cols=128, neg=INT_NEG, pos=E2M3_POS)
    for idt, odt in ((F32, F32), (F32, F16), (F16, F32), (F16, F16)):   # the generic kernels (fp16 -> fp16: with the clamp, off the fast path)
        for cols in (4, 8, 16, 32, 64, 128, 256, 512, 1024, 8192, 100, 102):
            if not (idt == F16 and odt == F16 and cols == 128):
                add(f"dual {idt}->{odt} c={cols}", "fpq_quant_rows_dual", rows=24, cols=cols, neg=E1M2_NEG, pos=E2M1_POS, in_dtype=idt, out_dtype=odt, flag=cols == 256,
                    clip=idt == F16 and odt == F16)
    # ---- codes
    for dt in (F16, F32):
        add(f"codes_mx in={dt}", "fpq_quant_rows_codes_mx", rows=40, cols=256, in_dtype=dt)
        add(f"absmax dt={dt}", "fpq_absmax", n=100000, dtype=dt)
        add(f"tensor_argmin in={dt}", "fpq_quant_tensor_argmin", n=100000, table_id=E2M1, in_dtype=dt)
        for t in (E1M2, E3M0):
            add(f"codes_g6 t={t} in={dt}", "fpq_quant_rows_codes_g6", rows=40, cols=256, table_id=t, in_dtype=dt)
        for pack in (0, 1):
            for cols in (128, 256):
                add(f"codes in={dt} c={cols} pack={pack}", "fpq_quant_rows_codes", rows=40, cols=cols, table_id=E2M1, in_dtype=dt, pack=pack)
            add(f"codes_segments in={dt} pack={pack}", "fpq_quant_rows_codes_segments", seg_rows=(24, 40, 8), cols=128, table_id=E2M1, in_dtype=dt, pack=pack)
            add(f"codes in={dt} pack={pack} FPQ_NO_FAST32", "fpq_quant_rows_codes", {"FPQ_NO_FAST32": 1}, rows=40, cols=128, table_id=E2M1, in_dtype=dt, pack=pack)
            add(f"codes_segments in={dt} pack={pack} FPQ_NO_FAST32", "fpq_quant_rows_codes_segments", {"FPQ_NO_FAST32": 1}, seg_rows=(24, 40, 8), cols=128,
                table_id=E2M1, in_dtype=dt, pack=pack)
            for odt in (F16, F32):
                for cols in (128, 256):
                    add(f"dequant s={dt} o={odt} c={cols} pack={pack}", "fpq_dequant_rows_codes", rows=40, cols=cols, table_id=E2M1, scale_dtype=dt, out_dtype=odt, pack=pack)
                add(f"dequant_segments s={dt} o={odt} pack={pack}", "fpq_dequant_rows_codes_segments", seg_rows=(24, 40, 8), cols=128, table_id=E2M1, scale_dtype=dt,
                    out_dtype=odt, pack=pack)
    add("codes_mx_km", "fpq_quant_rows_codes_mx_km", rows=40, cols=256, in_dtype=F16)
    # ---- fpq_rotate.hip
    for dt in (F16, F32):
        for name, t in (("e2m1", E2M1), ("e2m3", E2M3)):
            for smooth in (False, True):
                for rot in (False, True):
                    add(f"rotate in={dt} {name} smooth={smooth} rot_out={rot}", "fpq_rotate_quant_rows", rows=40, cols=1920, in_dtype=dt, table_id=t, smooth=smooth, rot_out=rot)
                    add(f"rotate in={dt} {name} smooth={smooth} rot_out={rot} FPQ_NO_HW4", "fpq_rotate_quant_rows", {"FPQ_NO_HW4": 1}, rows=40, cols=1920, in_dtype=dt,
                        table_id=t, smooth=smooth, rot_out=rot)
        for smooth in (False, True):
            for km in ("", "_km"):
                add(f"rotate_mx{km} in={dt} smooth={smooth}", "fpq_rotate_quant_rows_codes_mx" + km, rows=40, cols=1920, in_dtype=dt, smooth=smooth)
                add(f"rotate_mx{km} in={dt} smooth={smooth} FPQ_NO_HW4", "fpq_rotate_quant_rows_codes_mx" + km, {"FPQ_NO_HW4": 1}, rows=40, cols=1920, in_dtype=dt, smooth=smooth)
    for wgs in (2, 100000):
        add(f"rotate FPQ_ROT_WGS={wgs}", "fpq_rotate_quant_rows", {"FPQ_ROT_WGS": wgs}, rows=4096, cols=1920, in_dtype=F16, table_id=E2M1)
    for dt in (F16, F32):
        for cols in (512, 1024, 2048, 4096, 4104, 100):
            add(f"codes_fp8 in={dt} c={cols}", "fpq_quant_rows_codes_fp8", rows=40, cols=cols, table_id=E2M3, in_dtype=dt)
        for t in (E2M3, E3M2):
            for cols in (512, 2048, 4096, 8192, 8224):
                for km in (0, 1):
                    if not (km and cols % 128):
                        add(f"codes_f6 in={dt} t={t} c={cols} km={km}", "fpq_quant_rows_codes_f6", rows=40, cols=cols, table_id=t, in_dtype=dt, kmajor=km)
        add(f"codes_fp6 in={dt}", "fpq_quant_rows_codes_fp6", rows=40, cols=1920, table_id=E2M3, in_dtype=dt)
        add(f"codes_fp6_km in={dt}", "fpq_quant_rows_codes_fp6_km", rows=40, cols=1920, table_id=E2M3, in_dtype=dt)
    # ---- fpq_adaln.hip
    AD = "fpq_adaln_rotate_quant_"
    for cols in (512, 1024, 1536, 1920, 2304):      # MAXC 1 .. 5
        for opts in ({}, {"FPQ_NO_HW4": 1}, {"FPQ_NO_HW6": 1}, {"FPQ_ADALN_NO_PAIR2": 1}, {"FPQ_ADALN_NO_TIGHT": 1}):
            o = " ".join(opts)
            for name, t in SYM.items():
                if name in ("e2m1", "e2m3", "e3m2") or not opts:
                    add(f"adaln {name} c={cols} {o}", AD + "rows", opts, rows=40, cols=cols, table_id=t)
                    add(f"adaln emit {name} c={cols} {o}", AD + "rows", opts, rows=40, cols=cols, table_id=t, emit=True)
                    add(f"adaln token {name} c={cols} {o}", AD + "token_rows", opts, rows=40, cols=cols, table_id=t)
                    add(f"adaln token emit {name} c={cols} {o}", AD + "token_rows", opts, rows=40, cols=cols, table_id=t, emit=True)
            add(f"adaln mx c={cols} {o}", AD + "rows_codes_mx", opts, rows=40, cols=cols)
            add(f"adaln mx_km c={cols} {o}", AD + "rows_codes_mx_km", opts, rows=40, cols=cols)
            add(f"adaln token fp8 c={cols} {o}", AD + "token_rows_codes_fp8", opts, rows=40, cols=cols, table_id=E2M3)
            add(f"adaln token fp6 c={cols} {o}", AD + "token_rows_codes_fp6", opts, rows=40, cols=cols, table_id=E2M3)
            add(f"adaln token fp6_km c={cols} {o}", AD + "token_rows_codes_fp6_km", opts, rows=40, cols=cols, table_id=E2M3)
            add(f"adaln token f6 e3m2 c={cols} {o}", AD + "token_rows_codes_f6", opts, rows=40, cols=cols, table_id=E3M2, kmajor=0)
            add(f"adaln token f6 e3m2 km c={cols} {o}", AD + "token_rows_codes_f6", opts, rows=40, cols=cols, table_id=E3M2, kmajor=1)
        for idt, mdt in ((F16, F32), (F32, F16), (F32, F32)):
            ty = dict(in_dtype=idt, mod_dtype=mdt)
            for opts in ({}, {"FPQ_NO_HW4": 1}, {"FPQ_NO_HW6": 1}):
                o = f"in={idt} mod={mdt} " + " ".join(opts)
                for name in ("e2m1", "e2m3"):
                    for emit in (False, True):
                        add(f"adaln {name} emit={emit} c={cols} {o}", AD + "rows", opts, rows=40, cols=cols, table_id=SYM[name], emit=emit, **ty)
                        add(f"adaln token {name} emit={emit} c={cols} {o}", AD + "token_rows", opts, rows=40, cols=cols, table_id=SYM[name], emit=emit, **ty)
                add(f"adaln mx c={cols} {o}", AD + "rows_codes_mx", opts, rows=40, cols=cols, **ty)
            add(f"adaln token fp8 c={cols} in={idt} mod={mdt}", AD + "token_rows_codes_fp8", rows=40, cols=cols, table_id=E2M3, **ty)
    for cols in (1024, 1920):                        # rows per workgroup: 4 below 8192 rows, 8 from there, 12 from 32768 on for the issue-bound forms
        for rows in (8184, 8192, 32760, 32768):
            add(f"adaln e2m1 c={cols} r={rows}", AD + "rows", rows=rows, cols=cols, table_id=E2M1, rows_per_batch=rows)
            add(f"adaln e2m3 c={cols} r={rows}", AD + "rows", rows=rows, cols=cols, table_id=E2M3, rows_per_batch=rows)
            add(f"adaln mx c={cols} r={rows}", AD + "rows_codes_mx", rows=rows, cols=cols, rows_per_batch=rows)
            add(f"adaln e2m1 fp32 c={cols} r={rows}", AD + "rows", rows=rows, cols=cols, table_id=E2M1, rows_per_batch=rows, in_dtype=F32)
    for opts in ({"FPQ_ADALN_ROWS": 12}, {"FPQ_ADALN_ROWS": 7}, {"FPQ_ADALN_ROWS": 12, "FPQ_ADALN_TAIL": 120}, {"FPQ_ADALN_ROWS": 8, "FPQ_ADALN_TAIL": 60},
                 {"FPQ_ADALN_TAIL": 120}):
        o = " ".join(f"{k}={v}" for k, v in opts.items())
        for cols in (1024, 1920):
            add(f"adaln e2m1 c={cols} {o}", AD + "rows", opts, rows=7 * 53, cols=cols, table_id=E2M1, rows_per_batch=53)
            add(f"adaln e2m1 c={cols} r=8480 {o}", AD + "rows", opts, rows=160 * 53, cols=cols, table_id=E2M1, rows_per_batch=53)
    for cols in (2688, 4096):                        # rows beyond one wavefront: the first generation
        for rows in (40, 8200):
            add(f"adaln gen1 c={cols} r={rows}", AD + "rows", rows=rows, cols=cols, table_id=E2M1)
            add(f"adaln gen1 mx c={cols} r={rows}", AD + "rows_codes_mx", rows=rows, cols=cols)
        for idt, mdt in ((F16, F32), (F32, F16), (F32, F32)):
            add(f"adaln gen1 c={cols} in={idt} mod={mdt}", AD + "rows", rows=40, cols=cols, table_id=E2M1, in_dtype=idt, mod_dtype=mdt)
            add(f"adaln gen1 mx c={cols} in={idt} mod={mdt}", AD + "rows_codes_mx", rows=40, cols=cols, in_dtype=idt, mod_dtype=mdt)
    return R


class Walk:
    def __init__(self, lib_path):
        if lib_path:
            os.environ["FPQ_NO_NATIVE"] = "1"
        sys.path.insert(0, ROOT)
        import torch
        from fpqvar_amd import _lib
        self._lib, self.torch = _lib, torch
        self.lib = _lib.use_variant(lib_path) if lib_path else _lib.lib()
        dev = torch.device("cuda:0")
        z = lambda n: torch.zeros(n, dtype=torch.uint8, device=dev)
        self.buf = {"X": z(BIG), "OUT": z(BIG), **{k: z(SMALL) for k in "ABCDEF"}}
        self.keep = []    # device tables of segments: alive until the end of the walk
        self.sign = (ctypes.c_uint32 * 4)(0x12345678, 0x9ABCDEF0, 0x0F1E2D3C, 0x4B5A6978)
        torch.cuda.synchronize()

    def p(self, name, need, off=0):
        """address of buffer `name`, which the call may touch `need` bytes of"""
        if name is None:
            return None
        assert need + off <= self.buf[name].numel(), (name, need)
        return self.buf[name].data_ptr() + off

    def segments(self, struct, seg_rows, row_bytes, fields):
        """a device table of segments, each with its own slice of the buffers in `fields` ((field, buffer), ...)"""
        arr = (struct * len(seg_rows))()
        at = 0
        for i, r in enumerate(seg_rows):
            for f, b in fields:
                setattr(arr[i], f, self.p(b, at + r * row_bytes) + at)
            arr[i].rows = r
            at += (r * row_bytes + 255) // 256 * 256
        raw = bytes(arr)
        t = self.torch.frombuffer(bytearray(raw), dtype=self.torch.uint8).to(self.buf["X"].device)
        self.keep.append(t)
        return arr, t

    def call(self, entry, kw):
        L, p = self.lib, self.p
        g = kw.get
        rows, cols = g("rows", 0), g("cols", 0)
        full = rows * cols * 4 + 4096                    # what any one operand of the row may span
        sc = rows * cols // 8 + rows * 64 + 65536        # ... its scales (at most one fp32 per 32 elements, or per row)
        x = p("X", full, g("x_off", 0))
        idt, odt = g("in_dtype", F16), g("out_dtype", F16)
        if entry in ("fpq_quant_nearest", "fpq_quant_nearest_argmin"):
            return getattr(L, entry)(p("X", kw["n"] * 8), p("A", 1024), p("OUT", kw["n"] * 8), kw["n"], kw["k"], kw["dtype"], None)
        if entry == "fpq_quant_nearest_builtin":
            return L.fpq_quant_nearest_builtin(p("X", kw["n"] * 4), p("OUT", kw["n"] * 4), kw["n"], kw["table_id"], None)
        if entry == "fpq_quant_rows":
            return L.fpq_quant_rows(x, p("OUT", full), rows, cols, kw["table_id"], idt, odt, None)
        if entry == "fpq_quant_rows_multi":
            arr, _ = self.segments(self._lib.Segment, kw["seg_rows"], cols * 4 + 64, (("x", "X"), ("out", "OUT")))
            return L.fpq_quant_rows_multi(ctypes.cast(arr, ctypes.c_void_p), len(arr), cols, kw["table_id"], idt, odt, None)
        if entry == "fpq_quant_rows_segments":
            arr, t = self.segments(self._lib.Segment, kw["seg_rows"], cols * 4 + 64, (("x", "X"), ("out", "OUT")))
            return L.fpq_quant_rows_segments(t.data_ptr(), len(arr), max(kw["seg_rows"]), cols, kw["table_id"], idt, odt, None)
        if entry in ("fpq_quant_rows_codes_segments", "fpq_dequant_rows_codes_segments"):
            class Seg(ctypes.Structure):
                _fields_ = [("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("c", ctypes.c_void_p), ("rows", ctypes.c_int64)]
            arr, t = self.segments(Seg, kw["seg_rows"], cols * 4 + 64, (("a", "X"), ("b", "OUT"), ("c", "A")))
            if entry == "fpq_quant_rows_codes_segments":
                return L.fpq_quant_rows_codes_segments(t.data_ptr(), len(arr), max(kw["seg_rows"]), cols, kw["table_id"], idt, kw["pack"], None)
            return L.fpq_dequant_rows_codes_segments(t.data_ptr(), len(arr), max(kw["seg_rows"]), cols, kw["table_id"], kw["scale_dtype"], odt, kw["pack"], None)
        if entry.startswith("fpq_kv_cache_step"):
            batch, max_len, row_elems, n_new = 2, 24, 1024, 3
            cache = p("OUT", 2 * batch * max_len * row_elems * 2)
            new = (p("X", batch * n_new * row_elems * 2), p("A", batch * n_new * row_elems * 2))
            tail = (n_new * row_elems, row_elems, 9, n_new, kw["group"], kw["table_id"])
            if entry == "fpq_kv_cache_step":
                return L.fpq_kv_cache_step(cache, batch, max_len, row_elems, 2, 9, *new, *tail, None)
            return L.fpq_kv_cache_step_qknorm(cache, batch, max_len, row_elems, 2, 9, p("B", batch * n_new * row_elems * 2), *new, *tail,
                                              p("C", batch * n_new * row_elems * 2), p("D", row_elems), None, 64, None)
        if entry == "fpq_kv_pack":
            batch, max_len, heads, n_new = 2, 24, 16, 3
            return L.fpq_kv_pack(p("OUT", 2 * batch * max_len * heads * 48), p("B", 2 * batch * max_len * heads * 2), kw["kv_bit"], batch, max_len, heads, 64, 5,
                                 p("X", batch * n_new * heads * 128), p("A", batch * n_new * heads * 128), n_new * heads * 64, heads * 64, n_new, None)
        if entry == "fpq_quant_rows_argmin":
            return L.fpq_quant_rows_argmin(x, p("OUT", full), rows, cols, kw["table_id"], idt, kw["clamp3"], None)
        flag = p("B", 8) if g("flag") else None
        clip = p("C", 8) if g("clip") else None
        if entry == "fpq_quant_rows_dual":
            return L.fpq_quant_rows_dual(x, p("OUT", full), rows, cols, kw["neg"], kw["pos"], idt, odt, clip, 1.0, flag, None)
        if entry == "fpq_gelu_quant_rows_dual":
            return L.fpq_gelu_quant_rows_dual(x, p("OUT", full), p("A", full), rows, cols, kw["neg"], kw["pos"], flag, None)
        if entry == "fpq_quant_rows_neg_reverse":
            return L.fpq_quant_rows_neg_reverse(x, p("OUT", full), rows, cols, kw["table_id"], kw["dtype"], None)
        if entry == "fpq_quant_rows_dual_argmin":
            return L.fpq_quant_rows_dual_argmin(x, p("OUT", full), rows, cols, kw["neg"], kw["pos"], idt, None, 1.0, None)
        if entry in ("fpq_quant_rows_codes_mx", "fpq_quant_rows_codes_mx_km"):
            return getattr(L, entry)(x, p("OUT", full), p("A", full), rows, cols, idt, None)
        if entry == "fpq_absmax":
            return L.fpq_absmax(p("X", kw["n"] * 4), kw["n"], kw["dtype"], p("OUT", 4), None)
        if entry == "fpq_quant_tensor_argmin":
            return L.fpq_quant_tensor_argmin(p("X", kw["n"] * 4), p("OUT", kw["n"] * 4), p("A", 4), p("B", 8192), kw["n"], kw["table_id"], idt, None)
        if entry == "fpq_quant_rows_codes":
            return L.fpq_quant_rows_codes(x, p("OUT", full), p("A", full), rows, cols, kw["table_id"], idt, kw["pack"], None)
        if entry == "fpq_dequant_rows_codes":
            return L.fpq_dequant_rows_codes(x, p("A", full), p("OUT", full), rows, cols, kw["table_id"], kw["scale_dtype"], odt, kw["pack"], None)
        if entry in ("fpq_quant_rows_codes_g6", "fpq_quant_rows_codes_fp8", "fpq_quant_rows_codes_fp6", "fpq_quant_rows_codes_fp6_km"):
            return getattr(L, entry)(x, p("OUT", full), p("A", full), rows, cols, kw["table_id"], idt, None)
        if entry == "fpq_quant_rows_codes_f6":
            return L.fpq_quant_rows_codes_f6(x, p("OUT", full), p("A", full), rows, cols, kw["table_id"], idt, kw["kmajor"], None)
        smooth = p("F", cols * 4) if g("smooth") else None
        if entry == "fpq_rotate_quant_rows":
            return L.fpq_rotate_quant_rows(x, p("OUT", full), p("A", full) if g("rot_out") else None, rows, cols, idt, smooth, self.sign, kw["table_id"], None)
        if entry.startswith("fpq_rotate_quant_rows_codes_mx"):
            return getattr(L, entry)(x, p("OUT", full), p("A", sc), rows, cols, idt, smooth, self.sign, None)
        assert entry.startswith("fpq_adaln_rotate_quant_"), entry
        rpb = g("rows_per_batch", 8)
        n_batches = (rows + rpb - 1) // rpb
        mod = (idt, p("C", n_batches * cols * 4), p("D", n_batches * cols * 4), g("mod_dtype", F16), rpb, 1e-6, None, self.sign)
        h, y = (p("A", full), p("B", full)) if g("emit") else (None, None)
        form = entry[len("fpq_adaln_rotate_quant_"):]
        if form == "rows":
            return L.fpq_adaln_rotate_quant_rows(x, p("OUT", full), h, y, rows, cols, *mod, kw["table_id"], None)
        if form in ("rows_codes_mx", "rows_codes_mx_km"):
            return getattr(L, entry)(x, p("OUT", full), p("E", sc), rows, cols, *mod, None)
        if form == "token_rows":
            return L.fpq_adaln_rotate_quant_token_rows(x, p("OUT", full), h, y, p("E", sc), rows, cols, *mod, kw["table_id"], None)
        if form == "token_rows_codes_f6":
            return getattr(L, entry)(x, p("OUT", full), p("E", sc), rows, cols, *mod, kw["table_id"], kw["kmajor"], None)
        return getattr(L, entry)(x, p("OUT", full), p("E", sc), rows, cols, *mod, kw["table_id"], None)

    def run(self):
        table, refused = rows_table(), 0
        for label, entry, kw, opts in table:
            ctx = [self._lib.option(k, v) for k, v in opts.items()]
            for c in ctx:
                c.__enter__()
            try:
                rc = self.call(entry, kw)
            finally:
                for c in reversed(ctx):
                    c.__exit__(None, None, None)
            print(f"{label}: {entry} -> {rc}", flush=True)
            refused += rc != 0
        self.torch.cuda.synchronize()
        print(f"rows: {len(table)}  refused: {refused}  library: {self._lib.build_tag()}")


# ---- the comparison (no GPU) ----------------------------------------------------------------------------------------
def base_name(name):
    """a kernel's name without its parameter list and decorations, as both the profiler and the code objects spell it"""
    name = name.replace("(anonymous namespace)::", "").replace("half", "_Float16").strip().strip('"')
    name = re.sub(r"\.kd$", "", name)
    name = re.sub(r"^void ", "", name)
    depth = 0
    for i, ch in enumerate(name):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return name[:i].strip()
    return name.strip()


def trace(directory):
    """[(kernel, grid, workgroup, lds)] in dispatch order"""
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    assert len(files) == 1, (directory, files)
    with open(files[0], newline="") as f:
        recs = list(csv.DictReader(f))
    recs.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id", 0))))
    dims = lambda r, k: tuple(int(r[f"{k}_{a}"]) for a in "XYZ") if f"{k}_X" in r else int(r[k])
    # (the profiler leaves a name with _Float16 in it mangled: the code objects' demangler reads those)
    dem = _compare_kernels().demangle(sorted({r["Kernel_Name"] for r in recs if r["Kernel_Name"].startswith("_Z")}))
    return [(base_name(dem.get(r["Kernel_Name"], r["Kernel_Name"])), dims(r, "Grid_Size"), dims(r, "Workgroup_Size"), int(r["LDS_Block_Size"]))
            for r in recs]


def _compare_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import compare_kernels
    return compare_kernels


def producer_kernels(lib_path):
    """names of the kernels of the code objects that hold no matrix-core GEMM (fpq_gemm.hip's is the one that does)"""
    import tempfile
    ck = _compare_kernels()
    names = set()
    with tempfile.TemporaryDirectory() as tmp:
        for elf in ck.code_objects(lib_path, tmp):
            dem = ck.demangle(sorted(ck.figures(elf)))
            if not any(base_name(d).startswith("gemm_") for d in dem.values()):
                names |= {base_name(d) for d in dem.values()}
    return names


def compare(dir_a, dir_b, kernels_of):
    a, b = trace(dir_a), trace(dir_b)
    print(f"launches: {len(a)} and {len(b)}")
    diff = next((i for i, (u, v) in enumerate(zip(a, b)) if u != v), None if len(a) == len(b) else min(len(a), len(b)))
    if diff is None:
        print("identical: the same sequence of (kernel, grid, workgroup, LDS)")
    else:
        print(f"FIRST DIFFERENCE at launch {diff}:\n  {a[diff] if diff < len(a) else None}\n  {b[diff] if diff < len(b) else None}")
    if kernels_of:
        have = producer_kernels(kernels_of)
        seen = {k for k, _, _, _ in b}
        never = sorted(have - seen)
        print(f"kernels of the producer units: {len(have)}; launched by the walk: {len(have & seen)}; never launched: {len(never)}")
        for k in never:
            print(f"  {k}")
    return 0 if diff is None else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", help="another build of libfpq_hip.so (default: the stock one)")
    ap.add_argument("--compare", nargs=2, metavar="DIR")
    ap.add_argument("--kernels-of", help="with --compare: list the producer kernels of this library that the walk never launched")
    ap.add_argument("--list", action="store_true", help="print the rows and exit")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare, args.kernels_of))
    if args.list:
        for label, entry, kw, opts in rows_table():
            print(label, entry, kw, opts)
        sys.exit(0)
    Walk(args.lib).run()
