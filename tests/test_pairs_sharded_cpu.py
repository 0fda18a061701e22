"""sseq_de_pairs and merge_clusters over sharded matrices, without a device: the new entry points are declared,
mirrored and exported, the header says what is collective, the argument checks of the multi entry points that need no device, the
Python layer's signatures, the fixture of tests/test_gpu_sseq_pairs_sharded.py against the integer restatement (partial sums of any
cut add up, low words carry across ranks), and the limb scheme against Python integers."""
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
import pairs_sharded_case as pc  # noqa: E402
import sseq_pairs_ref as pref  # noqa: E402
import sseq_ref as ref  # noqa: E402

COLLECTIVE = ("scanrs_sseq_de_pairs_sharded", "scanrs_merge_clusters_sharded", "scanrs_cluster_medoids_sharded")
MULTI = ("scanrs_multi_sseq_de_pairs", "scanrs_multi_merge_clusters", "scanrs_multi_cluster_medoids")


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


@pytest.fixture(scope="module")
def case():
    return pc.make_case()


def test_the_new_entry_points_are_declared_mirrored_and_exported(sa):
    hdr = open(os.path.join(ROOT, "include", "scanrs_amd.h")).read()
    hpp = open(os.path.join(ROOT, "include", "scanrs_amd.hpp")).read()
    lib = ctypes.CDLL(sa.LIB_PATH)
    for name in COLLECTIVE:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*scanrs_mat \*m,", hdr), name
    for name in MULTI:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*scanrs_multi \*mm, int transposed,", hdr), name
    for name in COLLECTIVE + MULTI:
        assert name + "(" in hpp, name
        assert name in sa.EXPORTED_SYMBOLS and hasattr(lib, name), name
    pairs = open(os.path.join(ROOT, "scan-rs_amd", "csrc", "sseq_pairs.hip")).read()
    assert "pairs_acc_split_kernel" in pairs and "pairs_acc_join_kernel" in pairs
    cluster = open(os.path.join(ROOT, "scan-rs_amd", "csrc", "cluster.hip")).read()
    assert "medoid_dist_hist_kernel" in cluster and "medoid_dist_pick_kernel" in cluster


def test_the_header_says_what_is_collective_and_what_stays_refused():
    hdr = open(os.path.join(ROOT, "include", "scanrs_amd.h")).read()
    flat = lambda s: " ".join(s.replace("*", " ").split())  # noqa: E731
    for first, decl in (("scanrs_sseq_de_pairs over a sharded matrix", "int scanrs_sseq_de_pairs_sharded("),
                        ("merge_clusters and the medoids over a sharded matrix", "int scanrs_merge_clusters_sharded(")):
        doc = flat(hdr[hdr.index(first):hdr.index(decl)])
        for word in ("COLLECTIVE", "same arguments", "WHOLE matrix", "bit for bit", "dtype 1", "de_shard_allreduces", "de_shard_tests", "CELLS",
                     "unsharded handle"):
            assert word in doc, (first, word)
    # the plain entry points keep refusing a sharded handle, and the header keeps saying so
    de = flat(hdr[hdr.index("---- sSeq differential expression"):hdr.index("int scanrs_sseq_params(")])
    refused = de[de.index("What stays refused"):]
    for name in ("scanrs_sseq_de_pairs", "scanrs_merge_clusters", "column list"):
        assert name in refused, name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "7i" in design and "pairs_acc_split_kernel" in design and "medoid_dist_hist_kernel" in design


def _pairs_args(n=4):
    i16, u64, f64, u32 = (np.zeros(n, dtype=t) for t in (np.int16, np.uint64, np.float64, np.uint32))
    u32[0] = 1
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    # labels, n_groups, pair_a, pair_b, n_pairs, zeta, big_count, backend, snoop, 7 outputs, params
    return [p(i16), ctypes.c_uint32(2), p(u32), p(u32.copy()), ctypes.c_uint32(1), ctypes.c_double(0.995), ctypes.c_uint64(900), ctypes.c_int(0), None,
            p(u64), p(u64.copy()), p(f64), p(f64.copy()), p(f64.copy()), p(f64.copy()), p(f64.copy()), None], (i16, u64, f64, u32)


def test_argument_checks_of_the_multi_entry_points(sa):
    lib = sa._lib

    def err():
        return lib.scanrs_last_error().decode()

    args, keep = _pairs_args()
    assert lib.scanrs_multi_sseq_de_pairs(None, ctypes.c_int(0), *args) == 6 and "null" in err()
    bad = list(args)
    bad[7] = ctypes.c_int(2)
    assert lib.scanrs_multi_sseq_de_pairs(None, ctypes.c_int(0), *bad) == 6 and "backend" in err()
    for zeta in (1.5, -0.1, float("nan")):
        bad = list(args)
        bad[5] = ctypes.c_double(zeta)
        assert lib.scanrs_multi_sseq_de_pairs(None, ctypes.c_int(0), *bad) == 6 and "zeta_quintile" in err()
    i16, f64 = keep[0], keep[2]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.scanrs_multi_merge_clusters(None, ctypes.c_int(0), p(f64), ctypes.c_uint32(1), ctypes.c_uint32(1), p(i16), p(i16.copy()), None,
                                           None) == 6 and "null" in err()
    assert lib.scanrs_multi_cluster_medoids(None, ctypes.c_int(0), p(f64), ctypes.c_uint32(1), ctypes.c_uint32(1), p(i16), ctypes.c_uint32(1),
                                            p(f64.copy())) == 6 and "null" in err()
    assert lib.scanrs_sseq_de_pairs_sharded(None, *args) == 6 and "null" in err()
    assert lib.scanrs_merge_clusters_sharded(None, p(f64), ctypes.c_int(0), ctypes.c_uint32(1), ctypes.c_uint32(1), p(i16), p(i16.copy()), None,
                                             None) == 6 and "null" in err()


def test_the_python_layer_takes_a_multimat_and_transposed(sa):
    for fn in (sa.sseq_de_pairs, sa.sseq_de_each_vs_control, sa.merge_clusters, sa.cluster_medoids):
        par = inspect.signature(fn).parameters
        assert "transposed" in par and par["transposed"].default is False, fn.__name__
        assert par["mat"].annotation is inspect.Parameter.empty, fn.__name__  # an AdaptiveMat or a MultiMat
    for fn in (sa.sseq_de_pairs_sharded, sa.merge_clusters_sharded, sa.cluster_medoids_sharded):
        assert "transposed" not in inspect.signature(fn).parameters, fn.__name__


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
def test_the_fixture_is_what_the_gpu_tests_need(sa, case):
    mat, labels = case["mat"], case["labels"]
    genes, cells = mat.shape
    assert genes == 65 and 1200 <= cells <= 1300 and labels.shape == (cells,)
    tot = np.asarray(mat.sum(axis=0)).ravel()
    a, b = case["literal_pair"]
    assert ref.median(tot[(labels == a) | (labels == b)].astype(np.float64)) == 0.0  # the literal route
    assert np.count_nonzero(labels == b) <= 5 < np.count_nonzero(labels == a)  # a group made mostly of empty cells against a small one
    for pa, pb in case["pairs"]:
        if (pa, pb) != case["literal_pair"]:
            assert ref.median(tot[(labels == pa) | (labels == pb)].astype(np.float64)) > 0.0
    assert not np.any(labels == case["empty_group"]) and any(case["empty_group"] in pr for pr in case["pairs"])
    assert labels.max() == case["n_groups"] - 2 and labels.min() == -1
    indptr = sparse_csc_indptr(mat)
    for world in pc.SHARDS[1:]:
        bounds = [int(x) for x in sa.plan_shards(indptr, world)]  # the cut a MultiMat makes (host code: by nonzeros)
        one = np.flatnonzero(labels == case["one_shard_group"])
        assert bounds[-2] <= one.min() and len(one)  # one group lies inside a single shard
    bounds = [int(x) for x in sa.plan_shards(indptr, 5)]
    assert np.all(labels[bounds[1]:bounds[2]] == -1)  # one shard holds no labelled cell
    lo, hi = case["unlabelled_block"]
    assert lo <= bounds[1] and bounds[2] <= hi


def sparse_csc_indptr(mat):
    from scipy import sparse

    return sparse.csc_matrix(mat).indptr.astype(np.uint64)


def test_partial_sums_of_any_cut_add_up_and_low_words_carry(case):
    full = pref.GroupSums(case["mat"], case["labels"], case["n_groups"])
    n = len(full.s1)
    for world in (2, 3, 5):
        parts = pc.partial_sums(case, pc.cell_ranges(case["cells"], world))
        for name in ("x", "s1", "s2"):
            whole = getattr(full, name)
            assert all(sum(int(getattr(p, name)[i]) for p in parts) == int(whole[i]) for i in range(n)), (world, name)
        for name in ("s1", "s2"):  # a u64 sum of the low words alone would lose these carries
            carries = sum(1 for i in range(n) if sum(int(getattr(p, name)[i]) & pc.M64 for p in parts) > pc.M64)
            assert carries >= 1, (world, name)
        # the limb scheme on the fixture's own numbers: split per rank, summed as u64, joined
        for name in ("s1", "s2"):
            for i in range(n):
                words = [sum(w) for w in zip(*(pc.limb_split(int(getattr(p, name)[i])) for p in parts))]
                lo, hi = pc.limb_join(words)
                assert (hi << 64) | lo == int(getattr(full, name)[i]), (world, name, i)
    assert max(int(v) for v in full.s2) < 1 << 126 and max(int(v) for v in full.s1) < 1 << 126


def test_the_limb_scheme_against_python_integers():
    rng = np.random.default_rng(77)

    def rand128(bits):
        return int.from_bytes(rng.bytes(16), "little") >> (128 - bits)

    for trial in range(2000):
        # five partials whose sum stays below 2^126, the bound the pass's scale guarantees; every third trial with saturated low words
        parts = [rand128(int(rng.integers(1, 124))) for _ in range(5)]
        if trial % 3 == 0:
            parts = [(v >> 64 << 64) | (pc.M64 - int(rng.integers(0, 3))) for v in parts]
        words = [sum(w) for w in zip(*(pc.limb_split(v) for v in parts))]
        lo, hi = pc.limb_join(words)
        assert (hi << 64) | lo == sum(parts), (trial, parts)
    # the extreme of the scheme: 2^31 ranks that all contribute saturated halves still fit a u64 word
    assert (1 << 31) * pc.M32 <= pc.M64 and ((1 << 31) * pc.M32 >> 32) + (1 << 31) * pc.M32 <= pc.M64
