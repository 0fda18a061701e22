"""Restatement, in Python integers, of the fixed-point form of the f64 statistics over a list of columns whose sums cross the shards
of a sharded matrix (include/scanrs_amd.h, "THE QUANTUM"; scan-rs_amd/csrc/fixed128.hpp). The input is a DENSE f64
array of the mapped values of the view (zero where nothing is stored), so the functions know nothing of shards: the result of the
device must not depend on them either.

  quantum       scale = 2^(123 - ilogb(bound)), bound = M x T: M the largest finite |term| over the listed nonzeros, T the largest
                number of terms of a result (the longer list for the sum_rows family, the number of rows for sum_cols); for the sum
                of squares bound = (M x M) x T and the terms are the f64 products x * x
  a term        round-half-even(|t| x scale) as an integer, with the sign of t (to_fixed_signed)
  a sum         the exact integer sum
  the result    from_fixed_signed, operation by operation: f64(high word) x 2^64 + f64(low word), one rounding each, divided by
                the scale; NaN where a term was not finite"""
import math
from fractions import Fraction

import numpy as np

TWO64 = 18446744073709551616.0


def ilogb(x):
    return math.frexp(x)[1] - 1


def fx_scale(bound):
    """subset_host.cpp fx_scale / fixed128.hpp fixed_scale."""
    if not math.isfinite(bound):
        return math.nan
    if not bound > 0.0:
        return 1.0
    if ilogb(bound) < -877:
        return math.ldexp(1.0, 1000)
    return math.ldexp(1.0, 124 - ilogb(bound) - 1)


def to_fixed_signed(t, scale):
    """The integer a term becomes (|t| x scale is exact: the scale is a power of two)."""
    q = round(abs(float(t)) * scale)  # round(): half to even, an exact int
    return -q if t < 0.0 else q


def from_fixed_signed(total, scale):
    mag = abs(total)
    assert mag < 1 << 127
    hi, lo = mag >> 64, mag & ((1 << 64) - 1)
    v = (float(hi) * TWO64 + float(lo)) / scale
    return -v if total < 0 else v


def _max_term(terms):
    t = np.abs(terms[terms != 0.0])
    t = t[np.isfinite(t)]
    return float(t.max()) if t.size else 0.0


def _fixed_sum(terms, scale):
    """(result, flagged) of one sum over the nonzero entries of `terms`."""
    terms = terms[terms != 0.0]
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.abs(terms * scale) < 2.0 ** 125
    if not np.all(ok):
        return math.nan, True
    total = sum(to_fixed_signed(t, scale) for t in terms.tolist())
    return from_fixed_signed(total, scale), False


def _sums_of_lines(lines, scale, square=False):
    out = np.zeros(len(lines))
    for i, x in enumerate(lines):
        x = x[x != 0.0]
        out[i] = _fixed_sum(x * x if square else x, scale)[0]
    return out


def scales(dense, cols_union, n_terms):
    """(scale of the sums, scale of the sums of squares) of a call that lists `cols_union` and whose results have at most n_terms terms."""
    m = _max_term(np.asarray(dense)[:, cols_union])
    with np.errstate(over="ignore"):
        return fx_scale(m * float(n_terms)), fx_scale(np.float64(m) * np.float64(m) * float(n_terms))


def sum_rows(dense, cols):
    cols = np.asarray(cols, dtype=np.int64)
    s1, _ = scales(dense, cols, cols.size)
    return _sums_of_lines(np.asarray(dense)[:, cols], s1)


def sum_rows_dual(dense, cols1, cols2):
    c1, c2 = np.asarray(cols1, dtype=np.int64), np.asarray(cols2, dtype=np.int64)
    s1, _ = scales(dense, np.union1d(c1, c2).astype(np.int64), max(c1.size, c2.size))
    d = np.asarray(dense)
    return _sums_of_lines(d[:, c1], s1), _sums_of_lines(d[:, c2], s1)


def sum_cols(dense, cols):
    cols = np.asarray(cols, dtype=np.int64)
    d = np.asarray(dense)
    s1, _ = scales(d, cols, d.shape[0])
    return _sums_of_lines(d[:, cols].T, s1)


def mean_rows(dense, cols):
    with np.errstate(invalid="ignore", divide="ignore"):
        return sum_rows(dense, cols) / np.float64(len(cols))


def mean_var_rows(dense, cols, fused=False):
    """fused: the host line `var / len - mean * mean` with the product and the subtraction in ONE rounding (a compiler may contract
    it into a fused multiply-add; both are the same source line)."""
    cols = np.asarray(cols, dtype=np.int64)
    s1, s2 = scales(dense, cols, cols.size)
    sub = np.asarray(dense)[:, cols]
    s, sq = _sums_of_lines(sub, s1), _sums_of_lines(sub, s2, square=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.float64(cols.size)
        mean, e2 = s / n, sq / n
        if not fused:
            return mean, e2 - mean * mean
        var = np.array([float(Fraction(a) - Fraction(b) ** 2) if math.isfinite(a) and math.isfinite(b) else a - b * b
                        for a, b in zip(e2.tolist(), mean.tolist())])
        return mean, var
