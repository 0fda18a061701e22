"""hclust without a device: the reference's own tables through the host twin of the device chain, the ordering and cutting code on
scipy dendrograms against the restatement tests/hclust_ref.py, the twin against scipy and against an exact evaluation of the heights,
complete linkage against the library's linkage.rs port, and tied inputs.

Heights: the twin is held to max(16 eps, 8 x scipy's own largest relative deviation from the exact evaluation in np.longdouble of the
same case); the factor 8 covers the different order of Lance-Williams updates and Ward's square-then-root. Measured on the
development machine (largest relative deviation from the exact evaluation, in units of eps = 2.2e-16, scipy / twin):
    (65, 7):   single 0.95 / 0.95, complete 0.66 / 0.66, average 0.92 / 0.92, weighted 0.65 / 0.65, ward 1.34 / 0.96
    (257, 50): single 1.51 / 1.51, complete 1.67 / 1.67, average 2.48 / 2.48, weighted 1.51 / 1.51, ward 1.94 / 1.51
so every bound is 16 eps but (257, 50) average's 19.9 eps. Single and Complete heights are elements of the distance set on both sides.
The smallest relative gap between consecutive scipy heights (the precondition, >= 1e-9) was 1.6e-7 or more, at (1500, 16).
"""
import json
import os
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import hclust_ref as href  # noqa: E402

METHOD_NAMES = list(href.METHODS)


@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(TESTS, "golden", "hclust_reference_tables.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def hc():
    import scanrs_amd.hclust as hclust

    return hclust


@pytest.fixture(scope="module")
def scipy_cases():
    """scipy's dendrogram of every (shape, method), computed once."""
    out = {}
    for n, d in href.SHAPES:
        x = href.points(n, d)
        for m in METHOD_NAMES:
            out[(n, d, m)] = (x, href.scipy_steps(x, m))
    return out


def _twin_handle(hc, x, method):
    s = hc.host_linkage(x, method)
    return s, hc.HierarchicalCluster.from_steps(s.cluster1, s.cluster2, s.dissimilarity, s.size)


# ---- the reference's tables ----------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_tables(pins):
    assert href.relabel_vector(pins["relabel_input"]) == pins["relabel_expected"]
    c1, c2, ds, _ = href.scipy_steps(np.array(pins["array_3x10"], dtype=np.float64).T, "ward")
    for k, want in enumerate(pins["fcluster"]):
        assert href.fcluster(c1, c2, ds, k) == want, k
    c1, c2, ds, _ = href.scipy_steps(np.array(pins["array_2x10"], dtype=np.float64).T, "ward")
    assert href.leaves(c1, c2, ds, 0) == pins["leaves_naive"]
    assert href.leaves(c1, c2, ds, 1) == pins["leaves_modular_smallest"]


def test_reference_tables_through_the_host_twin(pins, hc):
    # ClusterDirection::Columns: the observations are the columns of the f32 arrays
    _, h = _twin_handle(hc, np.array(pins["array_3x10"], dtype=np.float32).T, "ward")
    for k, want in enumerate(pins["fcluster"]):
        assert h.fcluster(k).tolist() == want, k
    _, h = _twin_handle(hc, np.array(pins["array_2x10"], dtype=np.float32).T, "ward")
    assert h.leaves(hc.LeafOrdering.Naive).tolist() == pins["leaves_naive"]
    assert h.leaves(hc.LeafOrdering.ModularSmallest).tolist() == pins["leaves_modular_smallest"]


def test_relabel_vector_example_through_merge_below(pins, hc):
    # a dendrogram whose links below 2.0 make the example's partition {0, 2, 3}, {1}, {4, 6}, {5, 7}
    c1 = [0, 3, 4, 5, 1, 10, 12]
    c2 = [2, 8, 6, 7, 9, 11, 13]
    ds = [1.0, 1.0, 1.0, 1.0, 5.0, 5.0, 5.0]
    sz = [2, 3, 2, 2, 4, 4, 8]
    h = hc.HierarchicalCluster.from_steps(c1, c2, ds, sz)
    assert h.merge_clusters_below_distance_threshold(2.0).tolist() == pins["relabel_expected"]
    assert h.merge_clusters_below_distance_threshold(1.0).tolist() == list(range(1, 9))  # strictly below


@pytest.mark.parametrize("which", ["empty", "single"])
def test_fewer_than_two_observations_are_refused(pins, hc, which):
    import scanrs_amd as sa

    arr = np.array(pins["too_few"][which], dtype=np.float64).reshape(2, -1)
    with pytest.raises(sa.ScanrsError) as e:
        hc.host_linkage(arr.T, "ward")
    assert e.value.code == 1 and pins["too_few_message"] in str(e.value)


@pytest.mark.parametrize("method", ["centroid", "median"])
def test_centroid_and_median_are_not_provided(hc, method):
    import scanrs_amd as sa

    with pytest.raises(sa.ScanrsError) as e:
        hc.host_linkage(href.points(5, 2), method)
    assert e.value.code == 6 and method.capitalize() in str(e.value)


# ---- leaves, merge_below and fcluster on scipy dendrograms ------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHOD_NAMES)
@pytest.mark.parametrize("n", [2, 3, 65, 257])
def test_from_steps_on_scipy_dendrograms(hc, scipy_cases, n, method):
    d = dict(href.SHAPES)[n]
    _, (c1, c2, ds, sz) = scipy_cases[(n, d, method)]
    h = hc.HierarchicalCluster.from_steps(c1, c2, ds, sz)
    assert h.observations == n
    s = h.steps
    assert s.cluster1.tolist() == c1.tolist() and s.cluster2.tolist() == c2.tolist() and s.size.tolist() == sz.tolist()
    assert s.dissimilarity.tobytes() == ds.tobytes()
    for ordering in (0, 1):
        assert h.leaves(ordering).tolist() == href.leaves(c1, c2, ds, ordering)
    for k in sorted({0, 1, 2, 3, n // 2, n - 1, n, n + 1}):
        assert h.fcluster(k).tolist() == href.fcluster(c1, c2, ds, k), k
    for t in (0.0, float(ds[0]), float(ds[len(ds) // 2]), float(np.nextafter(ds[-1], np.inf)), np.inf):
        assert h.merge_clusters_below_distance_threshold(t).tolist() == href.merge_below(c1, c2, ds, t), t


def test_malformed_dendrograms_are_refused(hc):
    import scanrs_amd as sa

    good = ([0, 2, 3], [1, 4, 5], [1.0, 2.0, 3.0], [2, 3, 4])
    hc.HierarchicalCluster.from_steps(*good)
    bad = {
        "merged twice": ([0, 0, 3], [1, 4, 5], [1.0, 2.0, 3.0], [2, 3, 4]),
        "parent before child": ([0, 2, 3], [1, 5, 4], [1.0, 2.0, 3.0], [2, 3, 4]),
        "itself": ([0, 2, 5], [1, 4, 5], [1.0, 2.0, 3.0], [2, 3, 4]),
        "size": ([0, 2, 3], [1, 4, 5], [1.0, 2.0, 3.0], [2, 2, 4]),
        "unsorted": ([0, 2, 3], [1, 4, 5], [1.0, 3.0, 2.0], [2, 3, 4]),
        "nan": ([0, 2, 3], [1, 4, 5], [1.0, np.nan, 3.0], [2, 3, 4]),
        "out of range": ([0, 2, 3], [1, 4, 9], [1.0, 2.0, 3.0], [2, 3, 4]),
    }
    for why, steps in bad.items():
        with pytest.raises(sa.ScanrsError) as e:
            hc.HierarchicalCluster.from_steps(*steps)
        assert e.value.code == 6, why
    with pytest.raises(sa.ScanrsError) as e:
        hc.HierarchicalCluster.from_steps([], [], [], [])
    assert e.value.code == 1


# ---- the host twin against scipy -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHOD_NAMES)
@pytest.mark.parametrize("shape", href.SHAPES)
def test_host_twin_equals_scipy_structure(hc, scipy_cases, shape, method):
    n, d = shape
    x, (c1, c2, ds, sz) = scipy_cases[(n, d, method)]
    gap = href.min_relative_gap(ds)
    print(f"({n}, {d}) {method}: smallest relative gap between scipy's heights {gap:.3e}")
    assert gap >= 1e-9  # the precondition: the merge structure does not depend on rounding
    s = hc.host_linkage(x, method)
    href.check_dendrogram(s.cluster1, s.cluster2, s.dissimilarity, s.size)
    assert s.cluster1.tolist() == c1.tolist()
    assert s.cluster2.tolist() == c2.tolist()
    assert s.size.tolist() == sz.tolist()


@pytest.mark.parametrize("method", METHOD_NAMES)
@pytest.mark.parametrize("shape", [(65, 7), (257, 50)])
def test_host_twin_heights_against_the_exact_evaluation(hc, scipy_cases, shape, method):
    n, d = shape
    x, (c1, c2, ds, _) = scipy_cases[(n, d, method)]
    s = hc.host_linkage(x, method)
    assert s.cluster1.tolist() == c1.tolist() and s.cluster2.tolist() == c2.tolist()
    exact = href.exact_heights(x, method, s.cluster1, s.cluster2)
    dev_scipy = href.max_relative_deviation(ds, exact)
    dev_twin = href.max_relative_deviation(s.dissimilarity, exact)
    bound = max(16 * href.EPS, 8 * dev_scipy)
    print(f"({n}, {d}) {method}: scipy {dev_scipy / href.EPS:.2f} eps, twin {dev_twin / href.EPS:.2f} eps, bound {bound / href.EPS:.2f} eps")
    assert dev_twin <= bound


def test_complete_linkage_equals_the_linkage_rs_port(hc):
    import scanrs_amd as sa

    x = href.points(1025, 6)
    z = sa.linkage(x)
    s = hc.host_linkage(x, "complete")
    assert s.cluster1.tolist() == z[:, 0].astype(np.uint32).tolist()
    assert s.cluster2.tolist() == z[:, 1].astype(np.uint32).tolist()
    assert s.size.tolist() == z[:, 3].astype(np.uint32).tolist()
    assert s.dissimilarity.tobytes() == np.ascontiguousarray(z[:, 2]).tobytes()


# ---- ties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHOD_NAMES)
@pytest.mark.parametrize("case", ["symmetry5", "grid6"])
def test_tied_inputs_end_within_the_bound(hc, case, method):
    from scipy.cluster.hierarchy import linkage

    x = href.tie_cases()[case]
    s = hc.host_linkage(x, method)  # (SCANRS_ERR_NUMERICAL past 3 n steps)
    href.check_dendrogram(s.cluster1, s.cluster2, s.dissimilarity, s.size)
    if method == "single":
        assert s.dissimilarity.tobytes() == np.ascontiguousarray(linkage(x, "single")[:, 2]).tobytes()


def test_not_finite_input_is_refused_naming_the_element(hc):
    import scanrs_amd as sa

    x = href.points(7, 3)
    x[4, 1] = np.nan
    x[5, 0] = np.inf
    with pytest.raises(sa.ScanrsError) as e:
        hc.host_linkage(x, "average")
    assert e.value.code == 6 and "element 13 (row 4, column 1)" in str(e.value)


@pytest.mark.parametrize("method", METHOD_NAMES)
def test_overflowing_distances_are_refused(hc, method):
    """Finite input whose distances are not: refused by name, never carried into the chain (where a row without a finite entry has no
    nearest neighbour)."""
    import scanrs_amd as sa

    with pytest.raises(sa.ScanrsError) as e:
        hc.host_linkage(href.overflow_cases()["distance"], method)
    assert e.value.code == 6 and "observations 0 and 1" in str(e.value) and "overflow" in str(e.value)
    x = href.overflow_cases()["ward_update"]
    if method == "ward":
        with pytest.raises(sa.ScanrsError) as e:
            hc.host_linkage(x, method)
        assert e.value.code == 5 and "overflowed" in str(e.value)
    else:  # their updates stay within the largest distance times n
        s = hc.host_linkage(x, method)
        href.check_dendrogram(s.cluster1, s.cluster2, s.dissimilarity, s.size)
        assert np.all(np.isfinite(s.dissimilarity))


# ---- the interface -------------------------------------------------------------------------------------------------------------
def test_hclust_is_declared_mirrored_and_exported():
    import re

    import scanrs_amd as sa

    root = os.path.dirname(TESTS)
    hdr = open(os.path.join(root, "include", "scanrs_amd.h")).read()
    hpp = open(os.path.join(root, "include", "scanrs_amd.hpp")).read()
    names = ["scanrs_hclust_create", "scanrs_hclust_create_device", "scanrs_hclust_from_steps", "scanrs_hclust_free", "scanrs_hclust_n",
             "scanrs_hclust_steps", "scanrs_hclust_leaves", "scanrs_hclust_merge_below", "scanrs_hclust_fcluster", "scanrs_hclust_info",
             "scanrs_host_hclust_linkage", "scanrs_debug_hclust_pdist"]
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in scanrs_amd.h"
        assert name in hpp, f"{name} is not mirrored in scanrs_amd.hpp"
        assert name in sa.EXPORTED_SYMBOLS and hasattr(sa._lib, name)
    block = hdr[hdr.index("hclust: hierarchical clustering"):]
    for cite in ("132-148", "150-206", "210-227", "231-239", "122-125"):  # the header cites the reference's entry points
        assert cite in block
    assert "NOT provided: Centroid and Median" in block
    for name in ("HierarchicalCluster", "LinkageMethod", "ClusterDirection", "LeafOrdering"):
        assert hasattr(sa, name)
    assert [sa.LinkageMethod.Single, sa.LinkageMethod.Complete, sa.LinkageMethod.Average, sa.LinkageMethod.Weighted, sa.LinkageMethod.Ward,
            sa.LinkageMethod.Centroid, sa.LinkageMethod.Median] == list(range(7))  # kodama's order
    assert (sa.ClusterDirection.Rows, sa.ClusterDirection.Columns) == (0, 1)
    assert (sa.LeafOrdering.Naive, sa.LeafOrdering.ModularSmallest) == (0, 1)
