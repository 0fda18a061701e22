"""select_rows / select_cols / partition_on_thresholds over sharded matrices, without a device: the nine new entry
points are declared, mirrored and exported, the header names the new counter and says what is served and what stays refused, the
argument checks of the multi entry points that need no device, the Python layer's signatures, and the fixtures of
tests/test_gpu_select_sharded.py against the restatement tests/select_ref.py."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import select_ref as sref  # noqa: E402
import select_sharded_case as sc  # noqa: E402

NEW_SYMBOLS = {
    "scanrs_mat_select_rows_sharded": r"scanrs_mat \*m, const uint64_t \*idx, uint64_t n_idx, scanrs_mat \*\*out",
    "scanrs_mat_select_cols_sharded": r"scanrs_mat \*m, const uint64_t \*idx, uint64_t n_idx, scanrs_mat \*\*out",
    "scanrs_mat_partition_on_thresholds_sharded": r"scanrs_mat \*m, const double \*row_threshold, const double \*col_threshold,",
    "scanrs_mat_shard_info": r"const scanrs_mat \*m, uint32_t \*rank, uint32_t \*world, uint64_t \*outer_begin, uint64_t \*outer_global",
    "scanrs_multi_shape": r"const scanrs_multi \*mm, uint64_t \*rows, uint64_t \*cols, uint64_t \*nnz, int \*storage",
    "scanrs_multi_to_csmat": r"scanrs_multi \*mm, uint64_t \*indptr, uint32_t \*indices, uint32_t \*values",
    "scanrs_multi_select_rows": r"scanrs_multi \*mm, const uint64_t \*idx, uint64_t n_idx, scanrs_multi \*\*out",
    "scanrs_multi_select_cols": r"scanrs_multi \*mm, const uint64_t \*idx, uint64_t n_idx, scanrs_multi \*\*out",
    "scanrs_multi_partition_on_thresholds": r"scanrs_multi \*mm, const double \*row_threshold, const double \*col_threshold,",
}


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


def test_the_nine_entry_points_are_declared_mirrored_and_exported(sa):
    hdr = open(os.path.join(ROOT, "include", "scanrs_amd.h")).read()
    hpp = open(os.path.join(ROOT, "include", "scanrs_amd.hpp")).read()
    lib = ctypes.CDLL(sa.LIB_PATH)
    assert len(NEW_SYMBOLS) == 9
    for name, args in NEW_SYMBOLS.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + args, hdr), name
        assert name + "(" in hpp, name
        assert name in sa.EXPORTED_SYMBOLS and hasattr(lib, name), name
    counters = hdr[hdr.index("Event counters of the handle"):hdr.index("int scanrs_mat_get_counter(")]
    assert "partition_rounds" in counters and "partition_allreduces" in counters


def test_the_header_says_what_is_served_and_what_stays_refused():
    hdr = open(os.path.join(ROOT, "include", "scanrs_amd.h")).read()
    sel = hdr[hdr.index("---- select_rows / select_cols / partition_on_thresholds"):hdr.index("int scanrs_mat_to_csmat(")]
    doc = " ".join(sel.replace("*", " ").split())
    for word in ("COLLECTIVE", "WHOLE matrix", "scanrs_mat_shard_info", "outer_global", "LOCAL", "must not descend", "SCANRS_ERR_INVALID",
                 "bit for bit", "partition_allreduces", "dtype 1"):
        assert word in doc, word
    unchanged = doc[doc.index("Unchanged:"):doc.index("Transposed views work")]
    for name in ("column-list", "scanrs_sseq_de_pairs", "scanrs_merge_clusters", "stay refused", "scanrs_mat_to_adaptive", "own shard only"):
        assert name in unchanged, name
    multi = " ".join(hdr[hdr.index("int scanrs_multi_shape("):hdr.index("int scanrs_multi_select_rows(")].replace("*", " ").split())
    assert "NOT rebalanced" in multi and "either order" in multi and "NULL" in multi


def test_argument_checks_of_the_multi_entry_points(sa):
    lib = sa._lib

    def err():
        return lib.scanrs_last_error().decode()

    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    idx, lists = np.zeros(4, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    n_r, n_c = ctypes.c_uint64(), ctypes.c_uint64()
    out, res = ctypes.c_void_p(0x1234), ctypes.c_void_p(0x1234)
    thr = ctypes.c_double(3.0)
    for fn in (lib.scanrs_multi_select_rows, lib.scanrs_multi_select_cols):
        out.value = 0x1234
        assert fn(None, p(idx), ctypes.c_uint64(4), ctypes.byref(out)) == 6 and "null" in err()
        assert out.value is None  # *out is NULL on any failure
        assert fn(None, p(idx), ctypes.c_uint64(4), None) == 6 and "null" in err()
    assert lib.scanrs_multi_partition_on_thresholds(None, ctypes.byref(thr), ctypes.byref(thr), ctypes.byref(out), ctypes.byref(res), p(lists),
                                                    ctypes.byref(n_r), p(lists), ctypes.byref(n_c)) == 6 and "null" in err()
    assert out.value is None and res.value is None
    assert lib.scanrs_multi_shape(None, None, None, None, None) == 6 and "null" in err()
    assert lib.scanrs_multi_to_csmat(None, p(lists), None, None) == 6 and "null" in err()
    assert lib.scanrs_mat_shard_info(None, None, None, None, None) == 6 and "null" in err()
    assert lib.scanrs_mat_select_rows_sharded(None, p(idx), ctypes.c_uint64(4), ctypes.byref(out)) == 6 and "null" in err()
    assert lib.scanrs_mat_partition_on_thresholds_sharded(None, None, None, None, None, p(lists), ctypes.byref(n_r), p(lists), ctypes.byref(n_c)) == 6


def test_the_python_layer(sa):
    plain = inspect.signature(sa.AdaptiveMat.partition_on_thresholds)
    assert inspect.signature(sa.AdaptiveMat.partition_on_thresholds_sharded) == plain
    assert inspect.signature(sa.MultiMat.partition_on_thresholds) == plain
    assert inspect.signature(sa.AdaptiveMat.select_rows_sharded) == inspect.signature(sa.AdaptiveMat.select_rows)
    assert inspect.signature(sa.AdaptiveMat.select_cols_sharded) == inspect.signature(sa.AdaptiveMat.select_cols)
    for name in ("select_rows", "select_cols"):
        assert list(inspect.signature(getattr(sa.MultiMat, name)).parameters) == list(inspect.signature(getattr(sa.AdaptiveMat, name)).parameters)
    assert list(inspect.signature(sa.MultiMat.partition_on_threshold).parameters) == ["self", "threshold"]
    for name in ("shape", "nnz", "to_csmat", "to_scipy"):
        assert list(inspect.signature(getattr(sa.MultiMat, name)).parameters) == ["self"], name
    assert list(inspect.signature(sa.AdaptiveMat.shard_info).parameters) == ["self"]


def test_the_cascade_fixture():
    m, thr, rounds, gone = sc.cascade()
    assert m.shape == (15, 15) and rounds == 13 and list(gone) == list(range(12))
    ex_r, ex_c, r = sref.partition_sets(m, thr, thr)
    assert r == 13 and list(np.flatnonzero(ex_r)) == list(range(12)) and list(np.flatnonzero(ex_c)) == list(range(12))
    # one row and one column fall per round: every round's news is a single vector of each axis, so a sum or a flag that is not
    # exchanged in the round it belongs to stops the cascade
    for stop in range(1, 14):
        a, b = _after_rounds(m, thr, stop)
        assert list(np.flatnonzero(a)) == list(range(min(stop, 12))) and list(np.flatnonzero(b)) == list(range(min(stop, 12))), stop
    _, _, ef_rows, ef_cols, _ = sref.partition_on_thresholds(m, thr, thr)
    assert list(ef_rows) == [12, 13, 14] and list(ef_cols) == [12, 13, 14]
    f, r_, _, _, _ = sref.partition_on_thresholds(m, thr, thr)
    assert f.shape == (3, 3) and r_.shape == (3, 12) and r_.nnz == 2  # the two stray entries end up in the residual


def _after_rounds(m, thr, stop):
    """The masks of select_ref.partition_sets after `stop` rounds: how far the cascade has come."""
    csr = m.astype(np.int64)
    ex_r, ex_c = np.zeros(m.shape[0], dtype=bool), np.zeros(m.shape[1], dtype=bool)
    for _ in range(stop):
        ex_c |= np.asarray(csr.T @ (~ex_r).astype(np.int64)).ravel() < thr
        ex_r |= np.asarray(csr @ (~ex_c).astype(np.int64)).ravel() < thr
    return ex_r, ex_c


def test_the_seeded_fixture_has_one_case_of_each_kind():
    m = sc.seeded_matrix()
    assert m.shape == (sc.GENES, sc.CELLS) and m.nnz == sc.NNZ and m.data.min() == 1 and m.data.max() == 5
    per_gene, per_cell = np.diff(m.indptr), np.bincount(m.indices, minlength=sc.CELLS)
    empty = np.flatnonzero(per_cell == 0)  # (some of the thinned cells are empty as well)
    assert sorted(c for c in empty if not sc.THIN[0] <= c < sc.THIN[1]) == sorted(sc.EMPTY_CELLS)
    assert list(np.flatnonzero(per_gene == 0)) == [sc.EMPTY_GENE]
    thin = m[:, sc.THIN[0]:sc.THIN[1]]
    assert thin.nnz and thin.data.max() == 1 and thin.nnz < 0.05 * sc.GENES * (sc.THIN[1] - sc.THIN[0])
    kinds = set()
    for (rt, ct), (rounds, gone_r, gone_c) in sc.SEEDED_CASES.items():
        ex_r, ex_c, r = sref.partition_sets(m, rt, ct)
        assert (r, int(ex_r.sum()), int(ex_c.sum())) == (rounds, gone_r, gone_c), (rt, ct)
        if rt is not None and ct is not None and rounds > 2 and 0 < gone_r < sc.GENES and 0 < gone_c < sc.CELLS:
            kinds.add("several rounds, partial")
        if gone_r == sc.GENES and gone_c == sc.CELLS:
            kinds.add("total collapse")
        if rt is None and gone_c:
            kinds.add("columns only")
        if ct is None and gone_r:
            kinds.add("rows only")
    assert kinds == {"several rounds, partial", "total collapse", "columns only", "rows only"}
    # the excluded cells of the partial case lie in more than one fifth of the cells, and so do the kept ones: every cut into 2, 3 or 5
    # shards by nonzeros has news on both sides of a boundary
    _, ex_c, _ = sref.partition_sets(m, 34, 13)
    fifths = np.array_split(ex_c, 5)
    assert sum(bool(f.any()) for f in fifths) >= 3 and sum(bool((~f).any()) for f in fifths) >= 3
    labels = sc.seeded_labels()
    assert labels.min() == -1 and labels.max() == sc.N_GROUPS - 1 and labels.shape == (sc.CELLS,)
    assert sc.allreduce_bound(6, True, True) == 13 and sc.allreduce_bound(2, True, False) == 3
