"""CPU-side checks of the select / partition feature: the numpy / scipy restatement (tests/select_ref.py) against the reference
test's own dense procedure (sqz/src/mat.rs:1489-1562), and the new entry points in the headers and the Python package."""
import os
import re
import sys

import numpy as np
import pytest
from scipy import sparse

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import select_ref as sref  # noqa: E402

NEW_SYMBOLS = ["scanrs_mat_select_rows", "scanrs_mat_select_cols", "scanrs_mat_partition_on_thresholds", "scanrs_mat_to_csmat"]


def _random_matrix(rng, rows, cols):
    density = rng.uniform(0.01, 0.2)
    m = sparse.random(rows, cols, density=density, format="csr", random_state=np.random.RandomState(int(rng.integers(1 << 30))))
    m.data = rng.integers(1, 6, size=m.data.shape[0]).astype(np.int64)
    return m


@pytest.mark.parametrize("seed", range(6))
def test_restatement_matches_the_dense_procedure(seed):
    """Random matrices of the reference test's sizes (min dimension >= 100, up to 2 000), thresholds at the 0.1 quantile."""
    rng = np.random.default_rng(seed)
    rows, cols = (int(rng.integers(100, 2001)), int(rng.integers(100, 400))) if seed % 2 else (int(rng.integers(100, 400)), int(rng.integers(100, 2001)))
    m = _random_matrix(rng, rows, cols)
    dense = m.toarray()
    rt, ct = sref.quantile_threshold(dense.sum(axis=1)), sref.quantile_threshold(dense.sum(axis=0))
    f, r, sr, sc, rounds = sref.partition_on_thresholds(m, rt, ct)
    fd, rd, srd, scd, rounds_d = sref.partition_dense(dense, rt, ct)
    assert rounds == rounds_d
    assert np.array_equal(sr, srd) and np.array_equal(sc, scd)
    assert np.array_equal(f.toarray(), fd) and np.array_equal(r.toarray(), rd)
    assert f.shape != m.shape  # mat.rs:1557: the thresholds do remove something


def test_restatement_select_dense_and_sparse_agree():
    rng = np.random.default_rng(11)
    m = _random_matrix(rng, 300, 170)
    dense = m.toarray()
    for idx in (rng.integers(0, 300, 100), np.arange(300)[::3], rng.permutation(300), np.array([7]), np.arange(300), np.zeros(0, dtype=np.int64)):
        assert np.array_equal(sref.select_rows(m, idx).toarray(), sref.select_rows(dense, idx))
    for idx in (rng.integers(0, 170, 100), rng.permutation(170), np.array([0, 0, 169])):
        assert np.array_equal(sref.select_cols(m, idx).toarray(), sref.select_cols(dense, idx))


def test_cascade_matrix_is_a_cascade():
    a, gone_r, gone_c, rounds = sref.cascade_matrix()
    assert rounds >= 5 and len(gone_r) + len(gone_c) >= 4
    # only column 0 is below the threshold at the start
    assert list(np.flatnonzero(a.sum(axis=0) < 10)) == [0] and not (a.sum(axis=1) < 10).any()
    ex_r, ex_c, n = sref.partition_sets(sparse.csr_matrix(a), 10.0, 10.0)
    assert n == rounds and np.array_equal(np.flatnonzero(ex_r), gone_r) and np.array_equal(np.flatnonzero(ex_c), gone_c)
    assert sref.partition_dense(a, 10, 10)[4] == rounds


def test_one_sided_and_nan_thresholds():
    rng = np.random.default_rng(5)
    m = _random_matrix(rng, 150, 120)
    ex_r, ex_c, n = sref.partition_sets(m, None, None)
    assert n == 1 and not ex_r.any() and not ex_c.any()
    ex_r, ex_c, n = sref.partition_sets(m, float("nan"), float("nan"))
    assert n == 1 and not ex_r.any() and not ex_c.any()
    ct = sref.quantile_threshold(m.sum(axis=0))
    ex_r, ex_c, n = sref.partition_sets(m, None, ct)
    assert n == 2 and not ex_r.any() and np.array_equal(ex_c, np.asarray(m.sum(axis=0)).ravel() < ct)


def test_new_symbols_in_headers_package_and_library():
    import scanrs_amd as sa
    import ctypes

    hdr = open(os.path.join(ROOT, "include", "scanrs_amd.h")).read()
    hpp = open(os.path.join(ROOT, "include", "scanrs_amd.hpp")).read()
    lib = ctypes.CDLL(sa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in scanrs_amd.h"
        assert name in hpp, f"{name} is not mirrored in scanrs_amd.hpp"
        assert name in sa.EXPORTED_SYMBOLS and hasattr(lib, name)
    for method in ("select_rows", "select_cols", "partition_on_thresholds", "partition_on_threshold", "to_csmat", "to_scipy"):
        assert callable(getattr(sa.AdaptiveMat, method))
    assert '"partition_rounds"' in hdr
    for line in (207, 766, 1004):  # the header cites the reference's entry points
        assert str(line) in hdr[hdr.index("select_rows / select_cols / partition_on_thresholds"):]
