"""numpy model of fpq_packed_to_operands / fpq_operands_to_packed (include/fpq.h): the per-field maps between a packed file's table
INDEX and the GEMMs' hardware CODE for the five tables, the two dense packings, the decoders of the hardware formats, and the
k-major layout (dealt rows, chunk permutations) written down from the header's text - independent of the kernels' SWAR arithmetic."""
import numpy as np

FP4_TABLES, FP6_TABLES = ("e2m1", "e1m2", "e3m0"), ("e2m3", "e3m2")
TABLES = FP4_TABLES + FP6_TABLES
ZERO = {t: 7 for t in FP4_TABLES} | {t: 31 for t in FP6_TABLES}        # index of the level 0 in the sorted, de-duplicated table
SHIFT = {"e2m1": 0, "e1m2": 1, "e3m0": 2, "e2m3": 0, "e3m2": 0}        # magnitude index -> magnitude field of the code
SIGN = {"e2m1": 8, "e1m2": 32, "e3m0": 32, "e2m3": 32, "e3m2": 32}
CODE_FORMAT = {"e2m1": "e2m1", "e1m2": "e2m3", "e3m0": "e3m2", "e2m3": "e2m3", "e3m2": "e3m2"}   # the format that decodes the code


def code_of_index(table, idx):
    idx = np.asarray(idx, dtype=np.int64)
    z = ZERO[table]
    mag = np.abs(idx - z) << SHIFT[table]
    code = np.where(idx < z, SIGN[table] | mag, mag)
    return np.where(idx > 2 * z, 0, code).astype(np.uint8)


def index_of_code(table, code):
    code = np.asarray(code, dtype=np.int64)
    z = ZERO[table]
    mag = (code >> SHIFT[table]) & z
    return np.where(code & SIGN[table], z - mag, z + mag).astype(np.uint8)


def decode(fmt, code):
    """level of a hardware code: OCP E2M1 nibble, FP6 E2M3 (bias 1) or BF6 E3M2 (bias 3) field"""
    code = np.asarray(code, dtype=np.int64)
    ebits, mbits, bias = {"e2m1": (2, 1, 1), "e2m3": (2, 3, 1), "e3m2": (3, 2, 3)}[fmt]
    e, m = (code >> mbits) & ((1 << ebits) - 1), code & ((1 << mbits) - 1)
    mag = np.where(e == 0, m / 2.0 ** mbits * 2.0 ** (1 - bias), (1 + m / 2.0 ** mbits) * 2.0 ** (e.astype(np.float64) - bias))
    return np.where(code >> (ebits + mbits) & 1, -mag, mag).astype(np.float32)


def unpack4(b):
    b = np.asarray(b, dtype=np.uint8)
    return np.stack((b & 15, b >> 4), axis=-1).reshape(b.shape[0], -1)


def pack4(n):
    n = np.asarray(n, dtype=np.uint8).reshape(n.shape[0], -1, 2)
    return (n[..., 0] | (n[..., 1] << 4)).astype(np.uint8)


def unpack6(b):
    b = np.asarray(b, dtype=np.uint32).reshape(b.shape[0], -1, 3)
    w = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return np.stack([(w >> s) & 63 for s in (0, 6, 12, 18)], axis=-1).reshape(b.shape[0], -1).astype(np.uint8)


def pack6(c):
    c = np.asarray(c, dtype=np.uint32).reshape(c.shape[0], -1, 4)
    w = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
    return np.stack((w & 255, (w >> 8) & 255, (w >> 16) & 255), axis=-1).reshape(c.shape[0], -1).astype(np.uint8)


def operands_rowmajor(table, packed):
    """file bytes [outs, k/2 | k*3/4] -> row-major operand bytes"""
    idx = unpack4(packed) if table in FP4_TABLES else unpack6(packed)
    code = code_of_index(table, idx)
    return pack4(code) if table == "e2m1" else pack6(code)


def packed_of_operands(table, w_codes):
    code = unpack4(w_codes) if table == "e2m1" else unpack6(w_codes)
    idx = index_of_code(table, code)
    return pack4(idx) if table in FP4_TABLES else pack6(idx)


def dealt_image(codes, seg):
    """include/fpq.h, K-MAJOR IMAGES, weight side: [k/128][rows rounded up to 64][seg], zero where row(j) >= rows"""
    rows, steps = codes.shape[0], codes.shape[1] // seg
    rows64 = (rows + 63) // 64 * 64
    img = np.zeros((steps, rows64, seg), dtype=np.uint8)
    src = codes.reshape(rows, steps, seg // 16, 16)
    for j in range(rows64):
        row = (j & ~63) + 4 * (j & 15) + ((j >> 4) & 3)
        if row >= rows:
            continue
        for p in range(seg // 16):
            c = p ^ (0, 2, 3, 1)[(j & 15) >> 2] if seg == 64 else (p - ((j >> 3) & 1)) % 6
            img[:, j, 16 * p:16 * p + 16] = src[row, :, c]
    return img


def scale_image(scales):
    rows, groups = scales.shape
    img = np.zeros((groups, (rows + 63) // 64 * 64), dtype=np.float32)
    img[:, :rows] = scales.astype(np.float32).T
    return img
