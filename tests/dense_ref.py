"""Inputs, exact references and the case grid for the dense f64-MFMA kernels (scan-rs_amd/csrc/panel_ops.hip, dense.hip,
dense_skinny.inc). tests/test_dense_ref_cpu.py checks this file and the dispatch on the host; tests/test_gpu_dense.py walks the
same grid on the device.

Two input classes:
  * int_inputs: integer-valued doubles, |v| <= 2**10. Every product and every partial sum of a Gram / GEMM over at most 2**21 rows
    is an integer below 2**53, so ANY order of the sums, with or without FMA, gives the exact result: comparisons are bitwise.
  * dyadic_inputs: a * 2**-20 with integer |a| < 2**24, magnitudes log-uniform. Products are exact in int64 (2**48 per product,
    rows <= 4300: 2**48 * 2**13 < 2**63); the double result is compared with the exact one under the standard bound
    gamma_K * (|X|^T |Y|), gamma_K = K u / (1 - K u), u = 2**-53.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

GRAM_WAVE, GRAM_VEC, GRAM_TILED = 1, 2, 3
GEMM_WAVE, GEMM_TILED, GEMM_SKINNY_LDS, GEMM_DIRECT = 1, 2, 3, 4
GRAM_NAMES = {GRAM_WAVE: "GRAM_WAVE", GRAM_VEC: "GRAM_VEC", GRAM_TILED: "GRAM_TILED"}
GEMM_NAMES = {GEMM_WAVE: "GEMM_WAVE", GEMM_TILED: "GEMM_TILED", GEMM_SKINNY_LDS: "GEMM_SKINNY_LDS", GEMM_DIRECT: "GEMM_DIRECT"}
# the profile's name of the kernel class behind each route
GRAM_PROFILE = {GRAM_WAVE: "gram_mfma_f64", GRAM_VEC: "gram_vec_f64", GRAM_TILED: "gram_tiled_mfma_f64"}
GEMM_PROFILE = {GEMM_WAVE: "gemm_nn_mfma_f64", GEMM_TILED: "gemm_tiled_mfma_f64", GEMM_SKINNY_LDS: "gemm_skinny_mfma_f64",
                GEMM_DIRECT: "gemm_skinny_mfma_f64"}

INT_MAX = 2 ** 10
DYADIC_BITS, DYADIC_SCALE = 24, 20
MAX_EXACT_ROWS = 4300
SURPLUS_ROWS = 3  # rows_alloc - rows: rows the kernels must not read into a result

# sym: Y is X itself (y = NULL). forced: the device test also runs the case with the route forced and compares bitwise.
GramCase = namedtuple("GramCase", "route rows n m ldx ldy sym forced")
# gemm_direct / x_skew: the option and the alignment under which the dispatcher reaches `route`
GemmCase = namedtuple("GemmCase", "route rows n m ldx ldw ldc ldo gemm_direct x_skew forced")
WcsCase = namedtuple("WcsCase", "n l rank ldx with_xc")


def even_up(v):
    return (v + 1) & ~1


# ---- the dispatch rules restated from the comments in dense.hip / panel_ops.hip -------------------------------------------------
def expected_gram_route(n, m, rows, ldx, ldy, side=False, skip=False):
    if m == 1 and n <= 128 and rows >= 4096 and not skip:
        return GRAM_VEC
    if not side and n >= 48 and m >= 48 and rows >= 2048 and ldx % 2 == 0 and ldy % 2 == 0:
        return GRAM_TILED
    return GRAM_WAVE


def expected_gemm_route(n, m, rows, ldx, aligned=True, side=False, gemm_direct=True):
    """(route, nt, groups)"""
    if gemm_direct and aligned and 1 <= m <= 4096 and n >= 16 and rows >= 64 and ldx % 2 == 0:
        groups = 1 if m <= 112 else (m + 63) // 64
        return GEMM_DIRECT, ((m + 15) // 16 + groups - 1) // groups, groups
    if not side and n >= 16 and m >= 48 and rows >= 2048:
        if (m - 1) % 128 < 64:  # the last (or only) 128-column tile would be at most half full
            return GEMM_SKINNY_LDS, 0, (m + 63) // 64
        return GEMM_TILED, 0, (m + 127) // 128
    nj = 1 if m <= 16 else 2 if m <= 32 else 4
    return GEMM_WAVE, nj, (m + 16 * nj - 1) // (16 * nj)


# ---- the grid ---------------------------------------------------------------------------------------------------------------
def _gram_cases():
    out = []
    # GRAM_WAVE: every rows x every (n, m); leading dimensions of both parities
    shapes = [(1, 1), (15, 17), (16, 16), (17, 33), (32, 31), (33, 1), (1, 40)]
    k = 0
    for rows in (1, 7, 8, 9, 65, 1000):
        for n, m in shapes:
            out.append(GramCase(GRAM_WAVE, rows, n, m, n + k % 3, m + (k // 3) % 3, False, False))
            k += 1
    for rows in (9, 1000):
        for n, ldx in ((1, 1), (16, 17), (33, 34)):
            out.append(GramCase(GRAM_WAVE, rows, n, n, ldx, ldx, True, False))
    out.append(GramCase(GRAM_WAVE, 70000, 3, 3, 4, 3, False, False))  # the splits = 1024 clamp with the rps rounding
    # GRAM_VEC: m = 1, y a column of a wider panel
    for n in (1, 63, 64, 65, 128):
        for rows in (4096, 4097, 4127):
            for ldy in (1, 7):
                out.append(GramCase(GRAM_VEC, rows, n, 1, n + (rows & 1), ldy, False, n == 65 and rows == 4127))
    # GRAM_TILED
    for rows, n, m in ((2048, 48, 48), (2049, 49, 129), (2063, 129, 49), (2305, 130, 257)):
        for pad in (0, 6):
            out.append(GramCase(GRAM_TILED, rows, n, m, even_up(n) + pad, even_up(m) + pad, False, pad == 6 and n == 49))
    for rows, n in ((2048, 48), (2049, 129), (2063, 130), (2305, 257)):  # symmetric: the strictly lower tiles are mirrored
        for pad in (0, 6):
            out.append(GramCase(GRAM_TILED, rows, n, n, even_up(n) + pad, even_up(n) + pad, True, False))
    out.append(GramCase(GRAM_WAVE, 2048, 48, 48, 49, 49, True, False))  # X == Y by pointer, ldx odd: one wave per tile
    out.append(GramCase(GRAM_TILED, 4200, 48, 48, 48, 48, False, False))  # several splits with a short last one
    return out


def _odd_ld(m, extra=0):
    return (m | 1) + 2 * extra


def _gemm_case(route, rows, n, m, k, gemm_direct, x_skew=0, forced=False):
    ldo = m + 3 - (k % 2)  # ldo > m, both parities
    return GemmCase(route, rows, n, m, even_up(n) + 2 * (k % 2), _odd_ld(m, k % 2), ldo + 2, ldo, gemm_direct, x_skew, forced)


def _gemm_cases():
    out = []
    # GEMM_WAVE: through gemm_direct = 0 with rows < 2048; every second one also forced under gemm_direct = 1
    ms, ns, rs = (1, 16, 17, 32, 33, 64, 65, 130), (1, 3, 4, 15, 16, 17, 35), (1, 15, 16, 17, 63, 64, 65)
    k = 0
    for i in range(8):
        out.append(_gemm_case(GEMM_WAVE, rs[i % 7], ns[i % 7], ms[i], k, 0, forced=k % 2 == 0))
        k += 1
    for i in range(8):
        out.append(_gemm_case(GEMM_WAVE, rs[(i + 5) % 7], ns[(i + 3) % 7], ms[i], k, 0, forced=k % 2 == 0))
        k += 1
    for m, n in ((17, 17), (33, 35), (65, 3), (130, 16)):
        out.append(_gemm_case(GEMM_WAVE, 65, n, m, k, 0, forced=True))
        k += 1
    # X not 16-byte aligned: the dispatcher leaves the direct form
    out.append(_gemm_case(GEMM_WAVE, 97, 33, 129, k, 1, x_skew=1))
    out.append(_gemm_case(GEMM_WAVE, 65, 17, 17, k + 1, 1, x_skew=1))
    out.append(_gemm_case(GEMM_SKINNY_LDS, 2049, 17, 48, k, 1, x_skew=1))
    # GEMM_DIRECT: nb = 1..4 (n), NT = 1..7 (m <= 112), 2, 2, 3, 4 groups (m > 112), rows around 32 per wave / 128 per workgroup
    ns, m1, m2, rs = (16, 17, 31, 32, 33, 47, 48, 49, 64), (1, 15, 16, 17, 32, 48, 64, 80, 96, 97, 112), (113, 128, 129, 200), \
        (64, 65, 95, 96, 97, 127, 128, 129)
    for i in range(11):
        out.append(_gemm_case(GEMM_DIRECT, rs[i % 8], ns[i % 9], m1[i], k, 1))
        k += 1
    for i in range(9):
        out.append(_gemm_case(GEMM_DIRECT, rs[(i + 4) % 8], ns[i], m1[(i + 5) % 11], k, 1))
        k += 1
    for i in range(4):
        out.append(_gemm_case(GEMM_DIRECT, rs[(i + 3) % 8], ns[(2 * i + 1) % 9], m2[i], k, 1))
        k += 1
    for n, m, rows in ((17, 113, 65), (49, 112, 129), (33, 129, 97), (16, 1, 64)):
        out.append(_gemm_case(GEMM_DIRECT, rows, n, m, k, 1))
        k += 1
    # the LDS forms: gemm_direct = 0 with rows >= 2048; every third one also forced under gemm_direct = 1
    rs, ns = (2048, 2049, 2303, 2305), (16, 17, 33)
    lds = ((48, GEMM_SKINNY_LDS), (64, GEMM_SKINNY_LDS), (65, GEMM_TILED), (128, GEMM_TILED), (129, GEMM_SKINNY_LDS),
           (192, GEMM_SKINNY_LDS), (193, GEMM_TILED))  # 192: the second tile would be half full; 193: 65 of 128 columns
    for shift in (0, 1, 2):
        for i, (m, route) in enumerate(lds):
            out.append(_gemm_case(route, rs[(i + shift) % 4], ns[(i + 2 * shift) % 3], m, k, 0, forced=k % 3 == 0))
            k += 1
    return out


def _wcs_cases():
    out = []
    ns, ls = (1, 255, 256, 257, 4100), (1, 2, 127, 128, 129, 130)
    k = 0
    for l in ls:
        for pad in (0, 4):
            out.append(WcsCase(ns[k % 5], l, (1, 3)[k % 2], even_up(l) + pad, l % 2 == 0 and k % 4 != 3))
            k += 1
    for n in ns:
        for rank in (1, 3):
            l = ls[k % 6]
            out.append(WcsCase(n, l, rank, even_up(l) + 4 * (k % 2), l % 2 == 0))
            k += 1
    return out


GRAM_CASES = _gram_cases()
GEMM_CASES = _gemm_cases()
WCS_CASES = _wcs_cases()

# the four (alpha, beta, mode) of the exact class: mode "none" (no Cin), "in_place", "separate" (Cin != Out, ldc != ldo), "nan" (a Cin
# full of NaN that beta == 0 must not read)
GEMM_SCALARS = ((1.0, 0.0, "none"), (-1.0, 1.0, "in_place"), (0.5, 2.0, "separate"), (2.0, 0.0, "nan"))


def case_id(c):
    if isinstance(c, GramCase):
        return f"{GRAM_NAMES[c.route]}-r{c.rows}-n{c.n}-m{c.m}-ld{c.ldx}x{c.ldy}" + ("-sym" if c.sym else "")
    if isinstance(c, GemmCase):
        return f"{GEMM_NAMES[c.route]}-r{c.rows}-n{c.n}-m{c.m}-d{c.gemm_direct}s{c.x_skew}"
    return f"wcs-n{c.n}-l{c.l}-q{c.rank}-ld{c.ldx}" + ("-xc" if c.with_xc else "")


def _seed(c, kind):
    return [hash(tuple(int(v) for v in c)) & 0xFFFFFFFF, {"int": 1, "dyadic": 2}[kind]]


# ---- input makers -----------------------------------------------------------------------------------------------------------
def int_inputs(rng, shape):
    """int64 integers with |v| <= 2**10 (as doubles they are exact, and so is every partial sum of their products)"""
    return rng.integers(-INT_MAX, INT_MAX + 1, size=shape, dtype=np.int64)


def dyadic_inputs(rng, shape):
    """int64 mantissas a, |a| < 2**24, magnitudes log-uniform, signs random; the values are a * 2**-20"""
    mag = np.floor(2.0 ** rng.uniform(0.0, DYADIC_BITS, size=shape)).astype(np.int64)
    mag = np.minimum(mag, 2 ** DYADIC_BITS - 1)
    return mag * rng.choice(np.array([-1, 1], dtype=np.int64), size=shape)


def to_f64(mant, kind):
    return mant.astype(np.float64) * (1.0 if kind == "int" else 2.0 ** -DYADIC_SCALE)


def embed(values, rows_alloc, ld, poison):
    """values (rows x cols) in the top-left corner of a rows_alloc x ld buffer; the padding columns and surplus rows hold NaN
    (poison) or zeros"""
    buf = np.full((rows_alloc, ld), np.nan if poison else 0.0)
    buf[: values.shape[0], : values.shape[1]] = values
    return buf


def exact_matmul(a, b):
    """(a @ b, |a| @ |b|) in int64, with the overflow bound asserted: no entry of either can reach 2**63"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.int64 and b.dtype == np.int64 and a.shape[1] == b.shape[0]
    amax = int(np.max(np.abs(a))) if a.size else 0
    bmax = int(np.max(np.abs(b))) if b.size else 0
    assert amax * bmax * max(1, a.shape[1]) < 2 ** 63, "int64 reference would overflow"
    return a @ b, np.abs(a) @ np.abs(b)


def gamma(k):
    u = 2.0 ** -53
    return k * u / (1.0 - k * u)


# ---- per-case data (computed once, shared, read-only) -----------------------------------------------------------------------
GramData = namedtuple("GramData", "x y exact absref")  # x, y: int64 mantissas (y is x for a symmetric case); exact = x^T y
GemmData = namedtuple("GemmData", "x w cin exact absref")  # exact = x @ w
WcsData = namedtuple("WcsData", "b x exact")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@lru_cache(maxsize=None)
def gram_data(c, kind):
    assert kind == "int" or c.rows <= MAX_EXACT_ROWS
    rng = np.random.default_rng(_seed(c, kind))
    make = int_inputs if kind == "int" else dyadic_inputs
    x = make(rng, (c.rows, c.n))
    y = x if c.sym else make(rng, (c.rows, c.m))
    exact, absref = exact_matmul(x.T.copy(), y)
    return GramData(*_frozen(x, y, exact, absref))


@lru_cache(maxsize=None)
def gemm_data(c, kind):
    rng = np.random.default_rng(_seed(c, kind))
    make = int_inputs if kind == "int" else dyadic_inputs
    x, w, cin = make(rng, (c.rows, c.n)), make(rng, (c.n, c.m)), make(rng, (c.rows, c.m))
    exact, absref = exact_matmul(x, w)
    return GemmData(*_frozen(x, w, cin, exact, absref))


@lru_cache(maxsize=None)
def wcs_data(c):
    rng = np.random.default_rng(_seed(c, "int"))
    b, x = int_inputs(rng, (c.n, c.rank)), int_inputs(rng, (c.n, c.l))
    exact, _ = exact_matmul(b.T.copy(), x)
    return WcsData(*_frozen(b, x, exact))


def first_per_route(cases, key=lambda c: c.route):
    """one case per value of key, the first in grid order"""
    seen = {}
    for c in cases:
        seen.setdefault(key(c), c)
    return list(seen.values())
