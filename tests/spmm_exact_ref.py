"""Inputs and references for the sparse product routes (tests/test_gpu_spmm_routes.py, tests/test_spmm_exact_ref_cpu.py).

Dyadic case: counts from COUNT_SET (both sides of the tile kernels' table limits 8 and 15 and of the 8-bit count), panel entries
integers in [-1024, 1024], scale factors 2**e with e in [-3, 3], maps raw / Scale(a) -> Square -> Scale(1 - a) / both scales in
front of Square, a rank-2 offset of quarters. Every term and every product is a multiple of 2**-GRID, and the sum of their
magnitudes per output element stays below 2**53 grid units (`DyadicRef.mag`, asserted by the CPU test), so an f64 sum is exact in
any order and grouping, with or without FMA: the reference is integer arithmetic on the grid (int64, which cannot overflow under
that bound; the CPU test repeats rows of it in Python integers).

Bounded case: logarithm maps with real factors. Terms, products and sums in np.longdouble (64-bit significand, asserted by the
CPU test); per output element the exact value, S = sum |t||x| and n = the number of stored terms. The bound of a route is
B = (n + 32) 2**-53 S: n for an f64 summation in any order and grouping (at most n roundings of partial sums, each at most 2**-53
of S to first order), 32 for a term's own roundings on the longest route: a 2-ulp logarithm twice (numerator and denominator of the
quotient table, 4 + 4 half-ulps), the quotient, the factor divided out and multiplied back (two scale products, the division, the
product back: 4), the panel scaling, the product with the panel entry, the scale behind the logarithm, the conversion of the
longdouble reference: 24 half-ulps in all, rounded up to the next power of two.

Hostile cases: matrices with empty vectors at 0, every tile size and its double, n - 1 and mid-tile on both axes (EMPTY_AT), whose
normalisations carry infinite scale factors at those positions; and panels with one non-finite row. The reference sums stored
terms only (sqz/src/prod.rs:138-146), so an infinite factor of an empty vector is never applied and a non-finite panel row reaches
only the vectors that store a nonzero in it."""
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

import scanrs_oracle as so

COUNT_SET = tuple(range(1, 16)) + (16, 17, 255, 256, 300)
GRID = 12  # exponents in [-3, 3]: terms are multiples of 2**-12 = (2**-3 2**-3)**2 (a case with exponents in [-e, e]: 2**-4e)
PANEL_MAX = 1024
DYADIC_MAPS = ("raw", "sq_axis0", "sq_axis1", "sq_both")
# (rows, cols, fill): around slot (32), group, tile and part edges; fills keep 2**53 grid units (test_spmm_exact_ref_cpu.py)
WIDE_SHAPES = ((33, 97, 0.5), (257, 2000, 0.05), (97, 20000, 0.01), (2000, 193, 0.1))
WIDE_L = (16, 50, 104, 105)
EMPTY_AT = (0, 7, 40, 48, 64, 80, 96, 128, 192)  # and n - 1: tile sizes 40 / 48 / 64 / 96, their doubles, mid-tile
U53 = 2.0 ** -53


# ---- dyadic ------------------------------------------------------------------------------------------------------------------
@dataclass
class DyadicCase:
    rows: int
    cols: int
    dense: np.ndarray  # uint32 counts
    er: np.ndarray     # exponents of the row factors
    ec: np.ndarray     # ... of the column factors
    u4: np.ndarray     # rows x 2, quarters
    v4: np.ndarray     # 2 x cols, quarters
    x: np.ndarray      # cols x 105 panel for dot (integers as f64)
    xl: np.ndarray     # 105 x rows panel for rdot
    grid: int = GRID
    csr: object = None  # a large case: the counts as scipy CSR (int64), `dense` is None
    empty_rows: tuple = ()  # a large case: rows and columns without a nonzero
    empty_cols: tuple = ()

    def coo(self):
        if self.csr is not None:
            m = self.csr.tocoo()
            return m.row.astype(np.int64), m.col.astype(np.int64), m.data.astype(np.int64)
        ri, ci = np.nonzero(self.dense)
        return ri, ci, self.dense[ri, ci].astype(np.int64)

    @property
    def shape(self):
        return (self.rows, self.cols)

    @property
    def fr(self):
        return np.ldexp(1.0, self.er)

    @property
    def fc(self):
        return np.ldexp(1.0, self.ec)

    @property
    def u(self):
        return self.u4 / 4.0

    @property
    def v(self):
        return self.v4 / 4.0


def dyadic_counts(rng, rows, cols, fill, empty_rows=0.1):
    d = np.zeros((rows, cols), dtype=np.uint32)
    mask = rng.random((rows, cols)) < fill
    d[mask] = rng.choice(np.array(COUNT_SET, dtype=np.uint32), size=int(mask.sum()))
    d[rng.random(rows) < empty_rows, :] = 0
    d[0, 0] = 1
    return d


def dyadic_case(rows, cols, fill, seed, dense=None, csr=None, emax=3, lmax=max(WIDE_L)):
    """csr given: a large case kept sparse (counts as scipy CSR); emax: the scale exponents lie in [-emax, emax]"""
    rng = np.random.default_rng(seed)
    if csr is None and dense is None:
        dense = dyadic_counts(rng, rows, cols, fill)
    return DyadicCase(rows, cols, dense, rng.integers(-emax, emax + 1, rows), rng.integers(-emax, emax + 1, cols), rng.integers(-4, 5, (rows, 2)),
                      rng.integers(-4, 5, (2, cols)), rng.integers(-PANEL_MAX, PANEL_MAX + 1, (cols, lmax)).astype(np.float64),
                      rng.integers(-PANEL_MAX, PANEL_MAX + 1, (lmax, rows)).astype(np.float64), grid=max(4 * emax, 4), csr=csr)


def narrow_counts(rng, rows, cols, nnz_min, heavy_row_share=0.0, empty_rows=(), empty_cols=()):
    """scipy CSR of counts from COUNT_SET with just over nnz_min nonzeros; heavy_row_share of them in row 0 (at most every column
    that is not empty); the rows and columns listed hold nothing"""
    avail = cols - len(empty_cols)
    heavy = min(int(nnz_min * heavy_row_share), avail)
    light_rows = rows - (1 if heavy else 0) - len(empty_rows)
    p = (nnz_min - heavy) * 1.002 / (light_rows * avail)
    mask = rng.random((rows, cols)) < p
    if heavy:
        mask[0] = False
        mask[0, np.setdiff1d(np.arange(cols), empty_cols)[rng.permutation(avail)[:heavy]]] = True
    mask[list(empty_rows), :] = False
    mask[:, list(empty_cols)] = False
    ri, ci = np.nonzero(mask)
    m = sp.csr_matrix((rng.choice(np.array(COUNT_SET, dtype=np.int64), size=ri.shape[0]), (ri, ci)), shape=(rows, cols))
    assert m.nnz > nnz_min and m.nnz < nnz_min * 1.01, m.nnz
    return m


def dyadic_apply(case, name, scale_op, square_op):
    """the map `name` through scale_op(axis, factors) and square_op(): the same calls serve a library handle and the oracle"""
    if name == "raw":
        return
    if name == "sq_only0":
        scale_op(0, case.fr)
        square_op()
        return
    if name == "sq_both":
        scale_op(0, case.fr)
        scale_op(1, case.fc)
        square_op()
        return
    a = 0 if name == "sq_axis0" else 1
    scale_op(a, case.fr if a == 0 else case.fc)
    square_op()
    scale_op(1 - a, case.fc if a == 0 else case.fr)


def dyadic_gpu(sa, g, case, name):
    dyadic_apply(case, name, lambda ax, f: g.compose_scale_axis(ax, f), lambda: g.apply(sa.FN_SQUARE))
    return g


def dyadic_oracle(case, name, storage=so.CSR):
    box = [so.AdaptiveMat.from_dense(case.dense, storage)]
    dyadic_apply(case, name, lambda ax, f: box.__setitem__(0, box[0].compose_map(so.MapOp(so.OP_SCALE_AXIS, axis=ax, a=f))),
                 lambda: box.__setitem__(0, box[0].apply(so.OP_SQUARE)))
    return box[0]


def dyadic_terms(case, name):
    """the mapped matrix in grid units: int64 CSR"""
    ri, ci, c = case.coo()
    er, ec = case.er[ri].astype(np.int64), case.ec[ci].astype(np.int64)
    if name == "raw":
        t = c << case.grid
    elif name == "sq_both":
        t = (c * c) << (2 * (er + ec) + case.grid)
    elif name == "sq_axis0":
        t = (c * c) << (2 * er + ec + case.grid)
    elif name == "sq_axis1":
        t = (c * c) << (2 * ec + er + case.grid)
    elif name == "sq_only0":  # Scale(axis 0) -> Square
        t = (c * c) << (2 * er + case.grid)
    else:
        raise ValueError(name)
    return sp.csr_matrix((t, (ri, ci)), shape=case.shape)


@dataclass
class DyadicRef:
    want: np.ndarray  # f64, exact
    mag: np.ndarray   # int64: sum of the magnitudes of every term (offset included) in grid units


def dyadic_ref(case, name, side, l, offset):
    """side "dot": A x[:, :l]; "rdot": xl[:l] A. A = map(counts) (+ u v)."""
    t = dyadic_terms(case, name)
    ta = abs(t)
    off = 1 << (case.grid - 4)  # a product of two quarters in grid units
    if side == "dot":
        x = case.x[:, :l].astype(np.int64)
        r, m = t @ x, ta @ np.abs(x)
        if offset:
            r = r + off * (case.u4 @ (case.v4 @ x))
            m = m + off * (np.abs(case.u4) @ (np.abs(case.v4) @ np.abs(x)))
    else:
        x = case.xl[:l].astype(np.int64)
        r, m = (t.T @ x.T).T, (ta.T @ np.abs(x).T).T
        if offset:
            r = r + off * ((x @ case.u4) @ case.v4)
            m = m + off * ((np.abs(x) @ np.abs(case.u4)) @ np.abs(case.v4))
    assert r.dtype == np.int64 and m.dtype == np.int64
    return DyadicRef(np.ldexp(r.astype(np.float64), -case.grid), m)


def dyadic_ref_python(case, name, side, l, offset, i, k):
    """element (i, k) of dyadic_ref(...).want's integer in Python arithmetic"""
    t = dyadic_terms(case, name).toarray().astype(object)
    off = 1 << (case.grid - 4)
    if side == "dot":
        s = sum(int(t[i, j]) * int(case.x[j, k]) for j in range(case.cols))
        if offset:
            s += off * sum(int(case.u4[i, q]) * sum(int(case.v4[q, j]) * int(case.x[j, k]) for j in range(case.cols)) for q in range(2))
    else:
        s = sum(int(case.xl[i, r]) * int(t[r, k]) for r in range(case.rows))
        if offset:
            s += off * sum(sum(int(case.xl[i, r]) * int(case.u4[r, q]) for r in range(case.rows)) * int(case.v4[q, k]) for q in range(2))
    return s


# ---- bounded -----------------------------------------------------------------------------------------------------------------
def real_counts(rng, rows, cols, fill, vmax=9, empty_rows=0.1):
    d = np.zeros((rows, cols), dtype=np.uint32)
    mask = rng.random((rows, cols)) < fill
    d[mask] = rng.integers(1, vmax, size=int(mask.sum()))
    d[rng.random(rows) < empty_rows, :] = 0
    d[0, 0] = 1
    return d


def flip_ops(ops):
    """the chain of the transposed matrix"""
    return [so.MapOp(o.kind, 1 - o.axis if o.kind == so.OP_SCALE_AXIS else o.axis, o.a, o.b, o.swap) for o in ops]


def chain_terms(ops, ri, ci, counts):
    """the chain of an (untransposed) oracle matrix at its stored nonzeros, in longdouble"""
    ld = np.longdouble
    x = counts.astype(ld)
    for o in ops:
        assert not o.swap
        if o.kind == so.OP_INTO:
            continue
        if o.kind == so.OP_SCALE_AXIS:
            x = np.asarray(o.a, dtype=np.float64).astype(ld)[ri if o.axis == 0 else ci] * x
        elif o.kind == so.OP_LN_1P:
            x = np.log1p(x)
        elif o.kind == so.OP_LOG2_1P:
            x = np.log2(ld(1) + x)
        elif o.kind == so.OP_LOG10_1P:
            x = np.log10(ld(1) + x)
        elif o.kind == so.OP_SQUARE:
            x = x * x
        else:
            raise ValueError(o.kind)
    return x


class BoundedRef:
    """exact (longdouble), s = sum |t||x| (longdouble), n = stored terms per output row broadcast over the columns"""

    def __init__(self, exact, s, n, bound=None, unit=None):
        self.exact, self.s, self.n = exact, s, n
        self.bound = ((n + 32.0) * U53 * s).astype(np.float64) if bound is None else bound  # B, rounded to f64 once
        self.unit = (U53 * s).astype(np.float64) if unit is None else unit                  # 2**-53 S

    def cut(self, rows=slice(None), cols=slice(None)):
        return BoundedRef(self.exact[rows, cols], self.s[rows, cols], self.n[rows, cols], self.bound[rows, cols], self.unit[rows, cols])


def row_sums(vals, starts, counts):
    out = np.zeros((counts.shape[0],) + vals.shape[1:], dtype=vals.dtype)
    nz = counts > 0
    if vals.shape[0]:
        out[nz] = np.add.reduceat(vals, starts[nz], axis=0)
    return out


def bounded_ref(dense, ops, x):
    """A x for A = the chain `ops` on the stored counts of `dense` (rows x cols), x cols x l: per element exact, S, n.
    (rdot: call it with dense.T, flip_ops(ops), xl.T and transpose the result.)"""
    ri, ci = np.nonzero(dense)  # row-major order: sorted by row
    t = chain_terms(ops, ri, ci, dense[ri, ci])
    counts = np.bincount(ri, minlength=dense.shape[0])
    starts = np.concatenate(([0], np.cumsum(counts)[:-1]))
    prod = t[:, None] * np.asarray(x, dtype=np.float64).astype(np.longdouble)[ci]
    exact, s = row_sums(prod, starts, counts), row_sums(np.abs(prod), starts, counts)
    return BoundedRef(exact, s, np.broadcast_to(counts[:, None].astype(np.float64), exact.shape))


def transposed(ref):
    return BoundedRef(ref.exact.T, ref.s.T, ref.n.T, ref.bound.T, ref.unit.T)


def error_ratios(got, ref):
    """(worst |err| / B, worst |err| / (2**-53 S)) over the elements with stored terms; elements without any must be exactly 0.
    The error is formed in longdouble and rounded to f64 once."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got.astype(np.longdouble) - ref.exact).astype(np.float64)
    live = ref.n > 0
    assert np.all(got[~live] == 0.0), "an output row without stored terms is not zero"
    if not live.any():
        return 0.0, 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r_b = np.where(err == 0.0, 0.0, err / ref.bound)[live]  # (S == 0 with an error: inf; a NaN result: NaN, caught below)
        r_u = np.where(err == 0.0, 0.0, err / ref.unit)[live]
    if np.isnan(r_b).any():
        return float("inf"), float("inf")
    return float(r_b.max()), float(r_u.max())


# ---- hostile -----------------------------------------------------------------------------------------------------------------
def empty_positions(n):
    return sorted({p for p in EMPTY_AT if p < n} | {n - 1})


def hostile_counts(rng, rows, cols, fill, vmax=9):
    d = np.zeros((rows, cols), dtype=np.uint32)
    mask = rng.random((rows, cols)) < fill
    d[mask] = rng.integers(1, vmax, size=int(mask.sum()))
    d[empty_positions(rows), :] = 0
    d[:, empty_positions(cols)] = 0
    return d


def inf_at_empty(rng, n, empties):
    f = rng.random(n) + 0.5
    f[empties] = np.inf
    return f


def nonfinite_panel_case(dense, x, r, values):
    """x with row r replaced by `values` (cycled over the columns); (panel, panel with the row zeroed, rows of A x that must be
    non-finite = the rows of `dense` with a stored nonzero in column r)"""
    bad, zeroed = np.array(x, dtype=np.float64), np.array(x, dtype=np.float64)
    bad[r, :] = np.resize(np.asarray(values, dtype=np.float64), x.shape[1])
    zeroed[r, :] = 0.0
    return bad, zeroed, np.nonzero(dense[:, r])[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
