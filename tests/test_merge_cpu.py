"""merge_clusters' host pieces without a device: the restatement tests/merge_ref.py and the library's pdist, complete linkage and
relabel_by_size against the reference's pinned tables (linkage.rs, stats.rs), and against each other bit for bit on random
inputs, ties included."""
import json
import os
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import merge_ref as mref  # noqa: E402


@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(TESTS, "golden", "linkage_reference_tables.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


@pytest.mark.parametrize("which", ["a", "b"])
def test_pdist_and_linkage_pins(pins, sa, which):
    x = np.array(pins[f"input_{which}"])
    tol = pins["tolerance"]
    for d in (mref.pdist(x), sa.pdist(x)):
        np.testing.assert_allclose(d, pins[f"pdist_{which}"], rtol=0, atol=tol)
    for z in (mref.linkage(x), sa.linkage(x)):
        np.testing.assert_allclose(z, pins[f"linkage_{which}"], rtol=0, atol=tol)


def test_median_mut_pins(pins):
    for case in pins["median_mut"]:
        got = mref.median_mut(case["input"])
        assert got == case["expected"] and type(got) is type(case["expected"]), case
    with pytest.raises(ValueError):
        mref.median_mut([])


def _assert_same_bits(a, b):
    assert a.shape == b.shape
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("seed", range(6))
def test_linkage_matches_restatement_bitwise(sa, seed):
    rng = np.random.default_rng(seed)
    m, d = int(rng.integers(2, 40)), int(rng.integers(1, 12))
    x = rng.standard_normal((m, d))
    if seed % 2:
        # duplicate points and repeated coordinates: tied distances, decided by the order of the scans
        x[rng.integers(0, m, m // 3)] = x[0]
        x = np.round(x, 1)
    _assert_same_bits(sa.pdist(x), mref.pdist(x))
    _assert_same_bits(sa.linkage(x), mref.linkage(x))


def test_linkage_small_and_degenerate(sa):
    assert sa.linkage(np.zeros((1, 3))).shape == (0, 4)
    assert sa.pdist(np.zeros((1, 3))).shape == (0,)
    x = np.array([[0.0, 1.0], [3.0, 5.0]])
    _assert_same_bits(sa.linkage(x), mref.linkage(x))
    np.testing.assert_array_equal(sa.linkage(x), [[0.0, 1.0, 5.0, 2.0]])
    x = np.ones((5, 2))  # every distance ties
    _assert_same_bits(sa.linkage(x), mref.linkage(x))
    with pytest.raises(sa.ScanrsError):
        sa.linkage(np.zeros((0, 2)))
    with pytest.raises(sa.ScanrsError):
        sa.linkage(np.array([[0.0, np.nan], [1.0, 2.0]]))


@pytest.mark.parametrize("seed", range(4))
def test_relabel_by_size_matches_restatement(sa, seed):
    rng = np.random.default_rng(seed)
    lab = rng.integers(-3, 9, 200).astype(np.int16)
    np.testing.assert_array_equal(sa.relabel_by_size(lab), mref.relabel_by_size(lab))


def test_relabel_by_size_ties_keep_label_order(sa):
    lab = np.array([5, 5, 2, 2, 7, 7, 7, 0], dtype=np.int16)  # 7 largest; 2 and 5 tie (2 first); 0 last
    np.testing.assert_array_equal(sa.relabel_by_size(lab), [2, 2, 1, 1, 0, 0, 0, 3])
    np.testing.assert_array_equal(mref.relabel_by_size(lab), [2, 2, 1, 1, 0, 0, 0, 3])
    assert sa.relabel_by_size([]).shape == (0,)


def test_merge_header_documents_the_entry_points():
    hdr = open(os.path.join(os.path.dirname(TESTS), "include", "scanrs_amd.h")).read()
    for name in ("scanrs_host_pdist", "scanrs_host_linkage_complete", "scanrs_host_relabel_by_size", "scanrs_cluster_medoids",
                 "scanrs_cluster_medoids_device", "scanrs_merge_clusters", "scanrs_merge_trace", '"merge_fused"'):
        assert name in hdr, name
