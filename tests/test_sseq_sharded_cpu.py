"""sSeq differential expression over sharded matrices, without a device: the new entry points are declared, mirrored and exported, the
header says what a sharded handle is served and what stays refused, the argument checks of the multi entry points that need no device,
the Python layer's signatures, and the fixture of tests/test_gpu_sseq_sharded.py against the restatement (both branches occur)."""
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
import sseq_ref as ref  # noqa: E402
import sseq_sharded_case as sc  # noqa: E402

NEW_SYMBOLS = ("scanrs_multi_sseq_params", "scanrs_multi_group_sums", "scanrs_multi_sseq_de")


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


def test_the_new_entry_points_are_declared_mirrored_and_exported(sa):
    hdr = open(os.path.join(ROOT, "include", "scanrs_amd.h")).read()
    hpp = open(os.path.join(ROOT, "include", "scanrs_amd.hpp")).read()
    lib = ctypes.CDLL(sa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*scanrs_multi \*mm, int transposed,", hdr), name
        assert name + "(" in hpp, name
        assert name in sa.EXPORTED_SYMBOLS and hasattr(lib, name), name
    counters = hdr[hdr.index("Event counters of the handle"):hdr.index("int scanrs_mat_get_counter(")]
    assert "de_shard_tests" in counters and "de_shard_allreduces" in counters
    src = open(os.path.join(ROOT, "scan-rs_amd", "csrc", "sseq.hip")).read()
    assert "sseq_mom_split_kernel" in src and "sseq_mom_join_kernel" in src


def test_the_header_says_what_is_served_and_what_stays_refused():
    hdr = open(os.path.join(ROOT, "include", "scanrs_amd.h")).read()
    de = hdr[hdr.index("---- sSeq differential expression"):hdr.index("int scanrs_sseq_params(")]
    assert "Sharded handles return SCANRS_ERR_ARGUMENT" not in hdr
    doc = " ".join(de.replace("*", " ").split())
    for served in ("scanrs_sseq_params", "scanrs_mat_group_sums", "scanrs_sseq_de", "scanrs_sseq_de_backend"):
        assert served in doc, served
    assert "CELLS" in doc and "WHOLE matrix" in doc and "bit for bit" in doc and "outer_global" in doc
    refused = doc[doc.index("What stays refused"):]
    for name in ("scanrs_sseq_de_pairs", "scanrs_merge_clusters", "column list"):
        assert name in refused, name


def _de_args(n=4):
    i16, u64, f64, u8 = (np.zeros(n, dtype=t) for t in (np.int16, np.uint64, np.float64, np.uint8))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    # labels, n_groups, mode, size_factors, gene_means, gene_phi, use_genes, big_count, backend, snoop, 7 outputs
    return [p(i16), ctypes.c_uint32(2), ctypes.c_int(0), p(f64), p(f64), p(f64), p(u8), ctypes.c_uint64(900), ctypes.c_int(0), None, p(u64), p(u64),
            p(f64), p(f64), p(f64), p(f64), p(f64)], (i16, u64, f64, u8)


def test_argument_checks_of_the_multi_entry_points(sa):
    lib = sa._lib

    def err():
        return lib.scanrs_last_error().decode()

    args, keep = _de_args()
    assert lib.scanrs_multi_sseq_de(None, ctypes.c_int(0), *args) == 6 and "null" in err()
    bad = list(args)
    bad[2] = ctypes.c_int(3)
    assert lib.scanrs_multi_sseq_de(None, ctypes.c_int(0), *bad) == 6 and "mode" in err()
    bad = list(args)
    bad[8] = ctypes.c_int(2)
    assert lib.scanrs_multi_sseq_de(None, ctypes.c_int(0), *bad) == 6 and "backend" in err()
    f64, u8 = keep[2], keep[3]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    zh, dl = ctypes.c_double(), ctypes.c_double()
    assert lib.scanrs_multi_sseq_params(None, ctypes.c_int(0), ctypes.c_double(0.995), None, ctypes.c_uint64(0), None, p(f64), p(f64), p(f64), p(u8),
                                        p(f64), ctypes.byref(zh), ctypes.byref(dl), p(f64)) == 6 and "null" in err()
    assert lib.scanrs_multi_group_sums(None, ctypes.c_int(0), p(keep[0]), ctypes.c_uint32(2), p(keep[1]), None) == 6 and "null" in err()


def test_the_python_layer_takes_a_multimat_and_transposed(sa):
    for fn in (sa.compute_sseq_params, sa.group_sums, sa.sseq_differential_expression, sa.sseq_de_one_vs_rest, sa.sseq_de_vs_control):
        par = inspect.signature(fn).parameters
        assert "transposed" in par and par["transposed"].default is False, fn.__name__
    assert list(inspect.signature(sa.MultiMat.counter).parameters) == ["self", "key", "shard"]


def test_the_fixture_is_what_the_gpu_tests_need():
    case = sc.make_case()
    m, labels = case["mat"], case["labels"]
    assert m.shape == (sc.GENES, sc.CELLS) and m.dtype == np.uint32
    per_cell, per_gene = np.diff(m.indptr), np.bincount(m.indices, minlength=sc.GENES)
    assert sorted(np.flatnonzero(per_cell == 0)) == sorted(sc.EMPTY_CELLS) and list(np.flatnonzero(per_gene == 0)) == [sc.EMPTY_GENE]
    assert np.median(m.data) <= 15 and m.data.max() > 1000  # mostly 1 .. 15, a heavy tail
    cnt = np.bincount(labels[labels >= 0], minlength=sc.N_GROUPS)
    assert labels.min() == -1 and cnt[5] == 0 and np.all(cnt[:5] > 0)
    assert np.flatnonzero(labels == 3).max() < 40
    assert 0.05 * sc.CELLS <= np.sum(labels == -1) <= 0.15 * sc.CELLS
    assert len(set(case["subset"].tolist())) == len(case["subset"]) and np.any(np.diff(case["subset"].astype(np.int64)) < 0)
    params = ref.compute_sseq_params(m)
    assert np.all(params["size_factors"][list(sc.EMPTY_CELLS)] == 0.0)
    for mode in (0, 1, 2):
        for big in sc.BIG_COUNTS:
            asym, exact, settled = sc.branch_counts(m, labels, params, mode, big)
            assert asym > 0 and exact > 0 and asym + exact + settled == sc.GENES * sc.n_tests(mode), (mode, big, asym, exact, settled)
