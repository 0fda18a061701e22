"""nearest_neighbors under euclidean, pearson and cosine distance on the device (knn_metric.hip): both routes
against the host twin bit for bit - indices and distance bit patterns -, the shapes at which the filter declines, the device-pointer
entry, the euclidean kind against scanrs_knn, and the refusals. The host twin itself is held to the plain-Python restatement of the
reference in tests/test_metric_knn_cpu.py."""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import metric_knn_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = ("euclidean", "pearson", "cosine")
UMAX = 0xFFFFFFFF


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@contextlib.contextmanager
def options(sa, exhaustive=0, min_points=32768):
    sa.set_global_option("knn_exhaustive", exhaustive)
    sa.set_global_option("knn_filter_min_points", min_points)
    try:
        yield
    finally:
        sa.set_global_option("knn_exhaustive", 0)
        sa.set_global_option("knn_filter_min_points", 32768)


def same(got, want, label):
    assert got[0].shape == want[0].shape and got[0].dtype == np.uint32, label
    assert np.array_equal(got[0], want[0]), (label, "indices")
    assert np.array_equal(bits(got[1]), bits(want[1])), (label, "distance bits")


# ---- the exhaustive route, every DMAX instance ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 8, 9, 16, 17, 32, 33, 52, 53, 64, 65, 128])
@pytest.mark.parametrize("n", [3, 257])
def test_the_exhaustive_route_equals_the_host_twin(sa, n, d):
    x = cases.special_points(n, d)
    with options(sa, exhaustive=1):
        for kind in KINDS:
            for k in (1, 15, 64, 65, 128, n + 3):
                if k > 128:  # the limit of scanrs_knn holds on the device (the host twin takes any k)
                    with pytest.raises(sa.ScanrsError, match="k must not exceed 128"):
                        sa.nearest_neighbors(x, k, kind)
                    continue
                same(sa.nearest_neighbors(x, k, kind), sa.host_nearest_neighbors(x, k, kind), (kind, n, d, k))
                assert not sa.debug_knn_last_stats()["filtered"]


# ---- the filtered route at its smallest shape ----------------------------------------------------------------------------------------
N_FILTER = 4096  # more than KF_CAP = 1024 points: at least one filter round; and >= 256 queries
_TWIN = {}


def twin(sa, kind, d, x, k):
    """the host twin once per data set: the answer for a smaller k is a prefix of the answer for a larger one"""
    key = (kind, x.shape, hash(x.tobytes()))
    if key not in _TWIN or _TWIN[key][0].shape[1] < k:
        _TWIN[key] = sa.host_nearest_neighbors(x, max(k, 64), kind)
    idx, dist = _TWIN[key]
    return idx[:, :k], dist[:, :k]


@pytest.mark.parametrize("kind", ["pearson", "cosine"])
@pytest.mark.parametrize("d", [2, 50, 58])
def test_the_filtered_route_equals_the_exhaustive_route_and_the_host_twin(sa, kind, d):
    x = cases.clustered_points(N_FILTER, d)
    for k in (15, 64):
        with options(sa, min_points=1024):
            first = sa.nearest_neighbors(x, k, kind)
            st = sa.debug_knn_last_stats()
            assert st["filtered"] and len(st["rounds"]) >= 1 and st["rounds"][-1]["stride"] == 1 and st["rounds"][-1]["points"] == N_FILTER, st
            if kind == "pearson" and d == 2:  # every row standardises to +-(1, -1) / sqrt 2: half the set ties at D = 0, far more than
                assert st["rounds"][-1]["overflowed"] > 0, st  # a list holds, so the overflow redo answers
            second = sa.nearest_neighbors(x, k, kind)
        with options(sa, exhaustive=1):
            plain = sa.nearest_neighbors(x, k, kind)
            assert not sa.debug_knn_last_stats()["filtered"]
        same(first, second, (kind, d, k, "two runs"))
        same(first, plain, (kind, d, k, "filtered against exhaustive"))
        same(first, twin(sa, kind, d, x, k), (kind, d, k, "filtered against the host twin"))


def _declines(sa, x, k, kind, label, min_points=1024):
    with options(sa, min_points=min_points):
        got = sa.nearest_neighbors(x, k, kind)
        assert not sa.debug_knn_last_stats()["filtered"], (label, "the filter should have declined")
    same(got, twin(sa, kind, x.shape[1], x, k), label)


def test_the_filter_declines_where_it_must(sa):
    base = cases.clustered_points(N_FILTER, 50)
    x = base.copy()
    x[1234] = 0.75  # one constant row: degenerate under pearson
    _declines(sa, x, 15, "pearson", "constant row")
    x = base.copy()
    x[1234] = 0.0  # one zero row: degenerate under cosine
    _declines(sa, x, 15, "cosine", "zero row")
    for kind in ("pearson", "cosine"):
        _declines(sa, cases.clustered_points(N_FILTER, 59), 15, kind, "d = 59")
        _declines(sa, base, 65, kind, "k = 65")
        _declines(sa, base[:255], 15, kind, "255 queries", min_points=0)
        for scale in (1e-130, 1e130):  # s_xx outside [2^-400, 2^400]
            x = base.copy()
            x[77] *= scale
            _declines(sa, x, 15, kind, f"row scaled by {scale}")
    # and the same shapes just inside take it
    with options(sa, min_points=0):
        sa.nearest_neighbors(base[:1025], 15, "cosine")
        assert sa.debug_knn_last_stats()["filtered"]
        x = base[:2048].copy()
        x[77] *= 1e-50
        got = sa.nearest_neighbors(x, 15, "pearson")
        assert sa.debug_knn_last_stats()["filtered"]
    same(got, twin(sa, "pearson", 50, x, 15), "a row of magnitude 1e-50 inside the window")


# ---- the device-pointer entry ---------------------------------------------------------------------------------------------------------
def test_device_points_with_a_leading_dimension_and_nan_behind_the_columns(sa):
    import torch

    x = cases.special_points(257, 50)
    t = torch.full((257, 64), float("nan"), dtype=torch.float64, device="cuda")
    t[:, :50] = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    for kind in KINDS:
        same(sa.nearest_neighbors_device(t.data_ptr(), 257, 64, 50, 15, kind), sa.host_nearest_neighbors(x, 15, kind), kind)
    with pytest.raises(sa.ScanrsError, match="leading dimension"):
        sa.nearest_neighbors_device(t.data_ptr(), 257, 49, 50, 15, "cosine")


def test_device_points_straight_from_a_pca(sa):
    import torch
    from scanrs_amd.synth import synth_counts

    m = synth_counts(n_cells=1500, n_genes=600, density=0.05, seed=11)
    g = sa.AdaptiveMat.from_csmat(m.shape[1], m.shape[0], sa.CSC, m.indptr, m.indices, m.data)
    _, res = sa.BkSvd().run_pca_device(sa.normalize(g, sa.Normalization.CellRanger), 10)
    cells = m.shape[0]
    v = torch.as_tensor(sa.DevArray(res.d_v, cells * res.ld_v), device="cuda:0").view(cells, res.ld_v)[:, : res.k].cpu().numpy()
    for kind in KINDS:
        got = sa.nearest_neighbors_device(res.d_v, cells, res.ld_v, res.k, 15, kind)
        same(got, sa.host_nearest_neighbors(v, 15, kind), kind)
    with options(sa, min_points=1024):  # 1500 scores through the filter
        got = sa.nearest_neighbors_device(res.d_v, cells, res.ld_v, res.k, 15, "pearson")
        assert sa.debug_knn_last_stats()["filtered"]
    same(got, sa.host_nearest_neighbors(v, 15, "pearson"), "filtered")


# ---- the euclidean kind ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,min_points", [(257, 32768), (N_FILTER, 1024)])
def test_euclidean_is_scanrs_knn_with_the_square_root_of_its_squared_distance(sa, n, min_points):
    import knn_sharded_ref as ks

    x = cases.clustered_points(n, 50)
    with options(sa, min_points=min_points):
        idx, dist = sa.nearest_neighbors(x, 15, "euclidean")
        assert sa.debug_knn_last_stats()["filtered"] == (n == N_FILTER)
        assert np.array_equal(idx, sa.knn(x, 15))
    same((idx, dist), sa.host_nearest_neighbors(x, 15, "euclidean"), n)
    sq = np.zeros((n, 15))  # the fma chain of scanrs_knn over the chosen pairs
    for j in range(50):
        t = x[idx.astype(np.int64), j] - x[:, j][:, None]
        sq = ks.fma(t, t, sq)
    assert np.array_equal(bits(dist), bits(np.sqrt(sq)))


# ---- refusals and empty shapes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_refusals_and_padding(sa, kind):
    import ctypes

    x = cases.clustered_points(300, 5)
    for bad, row in ((np.nan, 123), (np.inf, 7), (-np.inf, 299)):
        y = x.copy()
        y[row, 3] = bad
        y[299, 0] = bad
        with pytest.raises(sa.ScanrsError, match=f"row {row} ") as e:
            sa.nearest_neighbors(y, 4, kind)
        assert e.value.code == 6
    with pytest.raises(sa.ScanrsError, match="k must not exceed 128"):
        sa.nearest_neighbors(x, 129, kind)
    with pytest.raises(sa.ScanrsError, match="dimensions"):
        sa.nearest_neighbors(np.ones((5, 129)), 2, kind)
    idx, dist = sa.nearest_neighbors(x[:1], 4, kind)
    assert idx.shape == (1, 0) and dist.shape == (1, 0)
    idx, dist = sa.nearest_neighbors(x, 0, kind)
    assert idx.shape == (300, 0) and dist.shape == (300, 0)
    # the C entry points write n x k and pad from column min(k, n - 1) on
    kinds = {"euclidean": 0, "pearson": 1, "cosine": 2}
    for n, k in ((1, 4), (3, 5)):
        ci = np.zeros((n, k), dtype=np.uint32)
        cd = np.zeros((n, k))
        pts = np.ascontiguousarray(x[:n])
        assert sa._lib.scanrs_nearest_neighbors(pts.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(n), ctypes.c_uint32(5), ctypes.c_uint32(k),
                                                ctypes.c_int(kinds[kind]), ci.ctypes.data_as(ctypes.c_void_p), cd.ctypes.data_as(ctypes.c_void_p)) == 0
        assert np.all(ci[:, n - 1:] == UMAX) and np.all(np.isposinf(cd[:, n - 1:])) and np.all(ci[:, : n - 1] < n)
