"""hclust on the device (scan-rs_amd/csrc/hclust.hip, hclust_host.cpp): the distance pass bit for bit against numpy's ordered sum,
the device dendrogram against the host twin of the chain, the reference's tables and tied inputs, the refusals, cancellation and
repeatability.

The square root: on the MI355X the device square root was bit-equal to np.sqrt on every value of the distance test (1 119 554 of
them), i.e. it is correctly rounded, so that test asserts equality instead of 1 ulp.
Heights of the device dendrogram are therefore compared with the host twin's bit for bit (not through the exact-evaluation bound of
tests/test_hclust_cpu.py)."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import hclust_ref as href  # noqa: E402

METHOD_NAMES = list(href.METHODS)
GPU_SHAPES = href.SHAPES + [(4097, 16)]


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


@pytest.fixture(scope="module")
def hc(sa):
    import scanrs_amd.hclust as hclust

    return hclust


@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(TESTS, "golden", "hclust_reference_tables.json")) as f:
        return json.load(f)


def _same_steps(a, b):
    assert a.cluster1.tolist() == b.cluster1.tolist()
    assert a.cluster2.tolist() == b.cluster2.tolist()
    assert a.size.tolist() == b.size.tolist()
    assert a.dissimilarity.tobytes() == b.dissimilarity.tobytes()


# ---- the distance pass ---------------------------------------------------------------------------------------------------------
def _ordered_squared(x):
    """numpy's s += (b[:, k] - a[:, k])**2 over k in order, condensed in pdist's order."""
    n, d = x.shape
    i, j = np.triu_indices(n, 1)
    s = np.zeros(len(i))
    for k in range(d):
        t = x[j, k] - x[i, k]
        s += t * t
    return s


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("shape", [(2, 1), (65, 7), (257, 50), (1025, 3)])
def test_distance_pass_equals_the_ordered_sum(hc, shape, padded):
    n, d = shape
    x = href.points(n, d)
    want = _ordered_squared(x)
    arr = x
    if padded:  # ld > d, the padding filled with NaN
        arr = np.full((n, d + 3), np.nan)
        arr[:, :d] = x
    got = hc.debug_pdist(arr, True, d)
    assert got.tobytes() == want.tobytes()
    root = hc.debug_pdist(arr, False, d)
    exact = np.sqrt(want)
    off = int(np.count_nonzero(root != exact))
    print(f"{shape} padded={padded}: {off} of {len(exact)} device square roots differ from np.sqrt")
    assert root.tobytes() == exact.tobytes()


# ---- the device chain against its host twin -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twins(hc):
    cache = {}

    def get(shape, method):
        if (shape, method) not in cache:
            x = href.points(*shape)
            cache[(shape, method)] = (x, hc.host_linkage(x, method))
        return cache[(shape, method)]

    return get


@pytest.mark.parametrize("method", METHOD_NAMES)
@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_device_equals_host_twin(hc, twins, shape, method):
    import torch

    n, d = shape
    x, want = twins(shape, method)
    xt = np.ascontiguousarray(x.T)
    runs = {
        "host rows": lambda: hc.HierarchicalCluster(x, method, hc.ClusterDirection.Rows),
        "host columns": lambda: hc.HierarchicalCluster(xt, method, hc.ClusterDirection.Columns),
    }
    # device input, with a leading dimension beyond the width
    pad_r = torch.zeros((n, d + 2), dtype=torch.float64, device="cuda")
    pad_r[:, :d] = torch.from_numpy(x)
    pad_c = torch.zeros((d, n + 5), dtype=torch.float64, device="cuda")
    pad_c[:, :n] = torch.from_numpy(xt)
    torch.cuda.synchronize()
    runs["device rows"] = lambda: hc.HierarchicalCluster(hc.DeviceArray2(pad_r.data_ptr(), n, d, d + 2, pad_r), method, hc.ClusterDirection.Rows)
    runs["device columns"] = lambda: hc.HierarchicalCluster(hc.DeviceArray2(pad_c.data_ptr(), d, n, n + 5, pad_c), method, hc.ClusterDirection.Columns)
    for name, run in runs.items():
        h = run()
        _same_steps(h.steps, want)
        info = h.info()
        assert info["merges"] == n - 1, name
        assert info["chain_steps"] < 3 * n, name
        assert info["matrix_bytes"] == n * n * 8 and info["launches"] >= 2 * info["chain_steps"]
    assert h.leaves(hc.LeafOrdering.ModularSmallest).tolist() == href.leaves(want.cluster1, want.cluster2, want.dissimilarity, 1)


@pytest.mark.parametrize("method", ["average", "ward"])
def test_factors_of_a_pca_left_on_the_device(sa, hc, method):
    """The issue's device form: the rows of U (genes x k) and of V (cells x k) where the handle's last PCA left them, with their own
    leading dimensions, against the twin on the factors the same call delivered to the host."""
    from scanrs_amd.synth import synth_counts

    m = synth_counts(n_cells=700, n_genes=300, density=0.08, seed=11)  # cells x genes CSR
    gm = sa.AdaptiveMat.from_csmat(m.shape[1], m.shape[0], sa.CSC, m.indptr, m.indices, m.data)  # genes x cells, CSC
    nm = sa.normalize(gm, sa.Normalization.CellRanger)
    u, _, v = sa.BkSvd().run_pca(nm, 6)
    res = sa.pca_result_device(nm)
    for dev, host in ((hc.DeviceArray2.u_of(res), u), (hc.DeviceArray2.v_of(res), v)):
        assert (dev.rows, dev.cols) == host.shape and dev.ld >= dev.cols
        h = hc.HierarchicalCluster(dev, method, hc.ClusterDirection.Rows)
        _same_steps(h.steps, hc.host_linkage(host, method))
        assert h.info()["merges"] == host.shape[0] - 1


def test_reference_tables_on_the_device(pins, hc):
    h = hc.HierarchicalCluster(np.array(pins["array_3x10"], dtype=np.float32), "ward", hc.ClusterDirection.Columns)
    for k, want in enumerate(pins["fcluster"]):
        assert h.fcluster(k).tolist() == want, k
    h = hc.HierarchicalCluster(np.array(pins["array_2x10"], dtype=np.float32), hc.LinkageMethod.Ward, hc.ClusterDirection.Columns)
    assert h.leaves(hc.LeafOrdering.Naive).tolist() == pins["leaves_naive"]
    assert h.leaves(hc.LeafOrdering.ModularSmallest).tolist() == pins["leaves_modular_smallest"]


@pytest.mark.parametrize("method", METHOD_NAMES)
@pytest.mark.parametrize("case", ["symmetry5", "grid6"])
def test_tied_inputs_on_the_device(hc, case, method):
    from scipy.cluster.hierarchy import linkage

    x = href.tie_cases()[case]
    h = hc.HierarchicalCluster(x, method, hc.ClusterDirection.Rows)  # (SCANRS_ERR_NUMERICAL past 3 n steps)
    s = h.steps
    href.check_dendrogram(s.cluster1, s.cluster2, s.dissimilarity, s.size)
    assert h.info()["chain_steps"] < 3 * len(x)
    _same_steps(s, hc.host_linkage(x, method))
    if method == "single":
        assert s.dissimilarity.tobytes() == np.ascontiguousarray(linkage(x, "single")[:, 2]).tobytes()


# ---- refusals, cancellation, repeatability -----------------------------------------------------------------------------------------
def test_refusals(sa, hc, pins):
    x = href.points(9, 4)
    for method in ("centroid", "median"):
        with pytest.raises(sa.ScanrsError) as e:
            hc.HierarchicalCluster(x, method)
        assert e.value.code == 6 and method.capitalize() in str(e.value)
    bad = x.copy()
    bad[6, 2] = np.nan
    bad[7, 0] = -np.inf
    with pytest.raises(sa.ScanrsError) as e:
        hc.HierarchicalCluster(bad, "average")
    assert e.value.code == 6 and "element 26 (row 6, column 2)" in str(e.value)
    with pytest.raises(sa.ScanrsError) as e:  # the same array by columns: still named by its place in the array as given
        hc.HierarchicalCluster(bad, "average", hc.ClusterDirection.Columns)
    assert e.value.code == 6 and "element 26 (row 6, column 2)" in str(e.value)
    # finite coordinates whose squared differences overflow: refused after the distance pass, before any chain step is queued
    with pytest.raises(sa.ScanrsError) as e:
        hc.HierarchicalCluster(href.overflow_cases()["distance"], "ward")
    assert e.value.code == 6 and "observations 0 and 1" in str(e.value)
    # finite squared distances whose Ward update overflows: the update flags it, every later step returns at once
    with pytest.raises(sa.ScanrsError) as e:
        hc.HierarchicalCluster(href.overflow_cases()["ward_update"], "ward")
    assert e.value.code == 5 and "overflowed" in str(e.value)
    assert hc.HierarchicalCluster(href.overflow_cases()["ward_update"], "average").observations == 4
    for arr, direction in ((x[:1], hc.ClusterDirection.Rows), (x[:, :1], hc.ClusterDirection.Columns)):
        with pytest.raises(sa.ScanrsError) as e:
            hc.HierarchicalCluster(arr, "ward", direction)
        assert e.value.code == 1 and pins["too_few_message"] in str(e.value)


def _memory_in_use(sa):
    import ctypes

    v = ctypes.c_uint64()
    assert sa._lib.scanrs_device_memory_in_use(ctypes.byref(v)) == 0
    return v.value


def test_a_set_cancel_flag_leaves_nothing_behind(sa, hc):
    import ctypes

    x = href.points(300, 5)
    before = _memory_in_use(sa)
    snoop = sa.AtomicSnoop()
    snoop.cancel()
    keep = snoop._struct()
    h = ctypes.c_void_p(0xDEAD)
    code = sa._lib.scanrs_hclust_create(x.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(300), ctypes.c_uint64(5), ctypes.c_uint64(5), 0, 2,
                                        ctypes.byref(keep), ctypes.byref(h))
    assert code == 3 and h.value is None  # SCANRS_ERR_CANCELLED, no handle
    with pytest.raises(sa.CancellationError):
        hc.HierarchicalCluster(x, "average", snoop=snoop)
    assert snoop.history == []  # nothing was queued, nothing reported
    assert _memory_in_use(sa) == before
    # an untouched snoop sees progress rise to 1
    snoop = sa.AtomicSnoop()
    hc.HierarchicalCluster(x, "average", snoop=snoop)
    assert snoop.history and snoop.history[-1] == 1.0 and all(a <= b for a, b in zip(snoop.history, snoop.history[1:]))
    assert _memory_in_use(sa) == before


@pytest.mark.parametrize("method", ["average", "ward"])
def test_two_runs_give_identical_bytes(hc, twins, method):
    x, want = twins((1500, 16), method)
    a = hc.HierarchicalCluster(x, method).steps
    b = hc.HierarchicalCluster(x, method).steps
    _same_steps(a, b)
    _same_steps(a, want)
