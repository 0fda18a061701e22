"""to_adaptive without a device: the C ABI of the AdaptiveVec encoders is declared, mirrored and exported, and the host side of the
header that host and device share (scan-rs_amd/csrc/adaptive_choose.hpp behind scanrs_host_choose_storage) picks what the oracle's
restatement of `AdaptiveVec::choose_storage` (sqz/src/vec.rs:1086-1131) picks."""
import collections
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import adaptive_grid as ag  # noqa: E402
import adaptive_vec as av  # noqa: E402

NEW_SYMBOLS = ("scanrs_mat_to_adaptive", "scanrs_adaptive_export_info", "scanrs_adaptive_export_vecs", "scanrs_adaptive_export_free",
               "scanrs_host_choose_storage")


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


def test_the_export_interface_is_declared_mirrored_and_exported(sa):
    hdr = open(os.path.join(ROOT, "include", "scanrs_amd.h")).read()
    hpp = open(os.path.join(ROOT, "include", "scanrs_amd.hpp")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(sa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in scanrs_amd.h"
        assert name in hpp, f"{name} is not used by the C++ mirror"
        assert name in sa.EXPORTED_SYMBOLS
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert "typedef struct scanrs_adaptive_export scanrs_adaptive_export;" in code
    assert "class AdaptiveExport" in hpp and "to_adaptive(int force_kind = -1)" in hpp
    assert "vec.rs:1086" in hdr and "mat.rs:92" in hdr  # the reference interfaces the entry points stand for
    for method in ("to_adaptive_vecs", "adaptive_info"):
        assert callable(getattr(sa.AdaptiveMat, method))
    assert callable(sa.choose_storage) and tuple(sa.ADAPTIVE_KINDS) == tuple(av.KINDS)


def _oracle_min_size(length, values):
    """the second member of choose_storage's result: the smallest estimate among D3, D4, D8, D16, S3, S4 (vec.rs:1087-1118)"""
    return min([av._est_dense(w, length, values) for w in ("3", "4", "8", "16")] + [av._est_sparse(w, length, values) for w in ("3", "4")])


def test_host_choose_storage_equals_the_oracle_on_the_grid(sa):
    oracle_kinds = collections.Counter()
    for length, vecs in ag.grid().items():
        for _, values in vecs:
            want = av.choose_storage(length, values)
            oracle_kinds[want] += 1
            kind, min_size = sa.choose_storage(length, values)
            assert sa.ADAPTIVE_KINDS[kind] == want, (length, len(values), want)
            assert min_size == _oracle_min_size(length, values), (length, len(values))
    # the grid reaches every encoding (counted on the oracle's side: a regenerated grid cannot silently lose one)
    assert dict(oracle_kinds) == {"V": 50, "S4": 38, "D4": 30, "D16": 11, "D8": 6, "D3": 6, "S8": 5, "S3": 4}


def test_the_grid_covers_the_edges_it_is_there_for():
    """a condition on the inputs of tests/test_gpu_adaptive_export.py, checked on the oracle alone"""
    grid = ag.grid()

    def chosen_for_empty(length):
        return {av.AdaptiveVec.new(length, v, i).kind for i, v in grid[length] if len(i) == 0}

    # empty vectors: S4 at length 21, V at length 300 (what the reference's estimates give)
    assert chosen_for_empty(21) == {"S4"} and chosen_for_empty(300) == {"V"}
    # empty leading and trailing 256-index blocks, all four markers in one fallback list, many work chunks in one vector
    sparse = [av.AdaptiveVec.with_kind("S3", 5000, v, i).block_starts for i, v in grid[5000][5:10]]  # 20 entries over 20 blocks
    assert all(len(b) == 21 for b in sparse) and any(b[0] == b[1] for b in sparse) and any(b[-2] == b[-1] for b in sparse)
    vals = grid[70001][20][1]
    assert len(vals) == 70001 and all((vals >= t).any() and (vals < t).any() for t in (7, 15, 255, 65535))


def test_host_choose_storage_literal_cases(sa):
    """the cases of tests/test_adaptive_vec.py::test_choose_storage_follows_the_size_estimates, through the host function"""
    rng = np.random.default_rng(3)

    def pick(length, values):
        return sa.ADAPTIVE_KINDS[sa.choose_storage(length, np.asarray(values, dtype=np.uint32))[0]]

    assert pick(1000, np.zeros(0, dtype=np.uint32)) == "V"
    assert pick(2100, rng.integers(1, 6, size=2100)) == "D3"
    assert pick(2100, rng.integers(7, 14, size=2100)) == "D4"
    assert pick(2100, rng.integers(20, 200, size=2100)) == "D8"
    assert pick(2100, rng.integers(300, 60000, size=2100)) == "D16"
    assert pick(33000, rng.integers(1, 5, size=1000)) == "S3"
    assert pick(33000, rng.integers(8, 14, size=1000)) == "S4"
    assert pick(33000, rng.integers(30, 200, size=1000)) == "V"     # the S8 branch does not lower min_size (vec.rs:1120-1123)
    assert pick(33000, rng.integers(30, 200, size=10000)) == "S8"
    assert pick(1_000_000, [3, 9, 1]) == "V"


def test_host_choose_storage_rejects_null_arguments(sa):
    lib = sa._lib
    kind = ctypes.c_int()
    assert lib.scanrs_host_choose_storage(ctypes.c_uint64(10), None, ctypes.c_uint64(3), ctypes.byref(kind), None) == 6
    assert lib.scanrs_host_choose_storage(ctypes.c_uint64(10), None, ctypes.c_uint64(0), None, None) == 6
    assert lib.scanrs_host_choose_storage(ctypes.c_uint64(10), None, ctypes.c_uint64(0), ctypes.byref(kind), None) == 0
    assert lib.scanrs_mat_to_adaptive(None, ctypes.c_int(-1), None) == 6
