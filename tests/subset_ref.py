"""numpy restatement of the statistics over a list of columns (sqz/src/mat.rs:279-282, 333-374, 409-583) on a DENSE array, the
checker of tests/test_gpu_subset.py. An integer array holds raw counts: its sums are exact (uint64 arithmetic). A float array holds
the MAPPED values (zero where nothing is stored, as `to_dense` of the oracle's AdaptiveMat gives them): its sums are `math.fsum`
over the listed entries, the correctly rounded sum whatever order the device adds in."""
import math

import numpy as np


def check_cols(cols, n_cols):
    """The lists the entry points accept: strictly ascending, in range."""
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    assert cols.size == 0 or (cols.min() >= 0 and cols.max() < n_cols), "index out of range"
    assert np.all(np.diff(cols) > 0), "not strictly ascending"
    return cols


def _is_int(dense):
    return np.issubdtype(np.asarray(dense).dtype, np.integer)


def _fsum_lines(lines):
    return np.array([math.fsum(x[x != 0.0].tolist()) for x in lines], dtype=np.float64)


def sum_rows(dense, cols):
    """Per row, the sum over the listed columns (mat.rs:449-481)."""
    dense = np.asarray(dense)
    sub = dense[:, check_cols(cols, dense.shape[1])]
    if _is_int(dense):
        return sub.astype(np.uint64).sum(axis=1, dtype=np.uint64)
    return _fsum_lines(sub)


def sum_cols(dense, cols):
    """Per listed column, in list order, the sum over all rows (mat.rs:414-446)."""
    dense = np.asarray(dense)
    sub = dense[:, check_cols(cols, dense.shape[1])]
    if _is_int(dense):
        return sub.astype(np.uint64).sum(axis=0, dtype=np.uint64)
    return _fsum_lines(sub.T)


def sum_rows_dual(dense, cols1, cols2):
    """Two sum_rows; a column in both lists counts in both (mat.rs:484-583)."""
    return sum_rows(dense, cols1), sum_rows(dense, cols2)


def mean_rows(dense, cols):
    """sum_rows::<f64> / cols.len() (mat.rs:279-282); an empty list gives 0.0 / 0.0."""
    cols = check_cols(cols, np.asarray(dense).shape[1])
    s = sum_rows(np.asarray(dense, dtype=np.float64), cols)
    with np.errstate(invalid="ignore", divide="ignore"):
        return s / np.float64(cols.size)


def mean_var_rows(dense, cols):
    """Per row, mean and E[x^2] - E[x]^2 of the mapped values over the listed columns (mat.rs:333-374)."""
    dense = np.asarray(dense, dtype=np.float64)
    cols = check_cols(cols, dense.shape[1])
    sub = dense[:, cols]
    s = _fsum_lines(sub)
    s2 = np.array([math.fsum((x[x != 0.0] ** 2).tolist()) for x in sub], dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.float64(cols.size)
        mean = s / n
        return mean, s2 / n - mean * mean


def var_axis(dense, axis):
    """mean_var_axis(axis).1 (mat.rs:409-411): over dense.shape[axis] positions, zeros included."""
    dense = np.asarray(dense, dtype=np.float64)
    lines = dense.T if axis == 0 else dense
    n = np.float64(dense.shape[axis])
    mean = _fsum_lines(lines) / n
    s2 = np.array([math.fsum((x[x != 0.0] ** 2).tolist()) for x in lines], dtype=np.float64)
    return s2 / n - mean * mean
