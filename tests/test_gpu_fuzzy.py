"""fuzzy_simplicial_set on the device (fuzzy.hip) against the host twin, bit for bit in every output, over the grid of
tests/fuzzy_cases.py, through the host-array and the device-pointer entries; umap_graph against fuzzy_simplicial_set of
nearest_neighbors under the three distances and both search routes; the star and the k = 128 staging case; a repeat run; the
refusals; and the device memory the calls leave behind. The twin itself is held to the reference in tests/test_fuzzy_cpu.py."""
import contextlib
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuzzy_cases as cases  # noqa: E402
import metric_knn_cases as knn_cases  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = ("euclidean", "pearson", "cosine")
GRID_SIZES = (2, 3, 6, 65, 257, 1000, 1500)


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def in_use(sa):
    """what the library holds on the device once everything an earlier test dropped is collected and the allocator's cache is empty"""
    gc.collect()
    sa.release_cached_memory()
    return sa.device_memory_in_use()


def outputs(g, n_epochs):
    """every output of a graph, floats as bit patterns"""
    indptr, indices, values = g.to_csr()
    head, tail, w, eps = g.edges(n_epochs)
    assert g.edge_count(n_epochs) == len(w)
    return dict(shape=np.array(g.shape), nnz=np.array([g.nnz]), indptr=indptr, indices=indices, values=bits(values), sigmas=bits(g.sigmas),
                rhos=bits(g.rhos), head=head, tail=tail, weights=bits(w), epochs_per_sample=bits(eps))


def same(got, want, label):
    for key in want:
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (label, key)


@contextlib.contextmanager
def options(sa, exhaustive=0, min_points=32768):
    sa.set_global_option("knn_exhaustive", exhaustive)
    sa.set_global_option("knn_filter_min_points", min_points)
    try:
        yield
    finally:
        sa.set_global_option("knn_exhaustive", 0)
        sa.set_global_option("knn_filter_min_points", 32768)


_GRID = {}


def grid_by_size(sa):
    if not _GRID:
        for case in cases.grid(sa):
            _GRID.setdefault(case[1].shape[0], []).append(case)
    return _GRID


def device_lists(idx, dist, ld):
    """the lists in device memory with leading dimension ld; what lies behind column k is an index that does not exist / NaN"""
    import torch

    n, k = idx.shape
    ti = torch.full((n, ld), 0x7FFFFFF0, dtype=torch.int32, device="cuda")
    td = torch.full((n, ld), float("nan"), dtype=torch.float64, device="cuda")
    ti[:, :k] = torch.from_numpy(idx.view(np.int32)).cuda()
    td[:, :k] = torch.from_numpy(dist).cuda()
    torch.cuda.synchronize()
    return ti, td


@pytest.mark.parametrize("n", GRID_SIZES)
def test_the_device_equals_the_twin_over_the_grid(sa, n):
    before = in_use(sa)
    n_refused = 0
    for name, idx, dist, prm, n_epochs in grid_by_size(sa)[n]:
        k = idx.shape[1]
        ti, td = device_lists(idx, dist, k + 3)
        try:
            twin = sa.host_fuzzy_simplicial_set(idx, dist, **prm)
        except sa.ScanrsError as e:  # refused by the twin: by the device too, naming the same row
            for call in (lambda: sa.fuzzy_simplicial_set(idx, dist, **prm),
                         lambda: sa.fuzzy_simplicial_set_device(ti.data_ptr(), td.data_ptr(), n, k + 3, k, **prm)):
                with pytest.raises(sa.ScanrsError) as e2:
                    call()
                assert str(e2.value) == str(e), name
            n_refused += 1
            continue
        with twin, sa.fuzzy_simplicial_set(idx, dist, **prm) as g, \
                sa.fuzzy_simplicial_set_device(ti.data_ptr(), td.data_ptr(), n, k + 3, k, **prm) as gd:
            want = outputs(twin, n_epochs)
            same(outputs(g, n_epochs), want, (name, "host arrays"))
            same(outputs(gd, n_epochs), want, (name, "device pointers"))
            assert g.on_device and gd.on_device and not twin.on_device and all(g.device_pointers())
    assert in_use(sa) == before
    print(f"n = {n}: {len(grid_by_size(sa)[n])} cases, {n_refused} refused")


@pytest.mark.parametrize("kind", KINDS)
def test_umap_graph_equals_the_graph_of_nearest_neighbors_exhaustive(sa, kind):
    import torch

    x = cases.points(257, 10)
    t = torch.full((257, 16), float("nan"), dtype=torch.float64, device="cuda")
    t[:, :10] = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    before = in_use(sa)
    with options(sa, exhaustive=1):
        for k, prm in ((15, {}), (128, dict(local_connectivity=2.0, set_op_mix_ratio=0.5)), (300, dict(apply_fuzzy_combine=False, n_iter=3))):
            if k > 128:  # the width is min(k, n - 1) = 256, past the limit of both stages
                with pytest.raises(sa.ScanrsError, match="k must not exceed 128"):
                    sa.umap_graph(x, k, kind, **prm)
                continue
            idx, dist = sa.nearest_neighbors(x, k, kind)
            with sa.fuzzy_simplicial_set(idx, dist, **prm) as want, sa.umap_graph(x, k, kind, **prm) as g, \
                    sa.umap_graph_device(t.data_ptr(), 257, 16, 10, k, kind, **prm) as gd:
                assert not sa.debug_knn_last_stats()["filtered"]
                w = outputs(want, 200.0)
                same(outputs(g, 200.0), w, (kind, k, "umap_graph"))
                same(outputs(gd, 200.0), w, (kind, k, "umap_graph_device"))
    assert in_use(sa) == before


def test_umap_graph_width_is_capped_at_n_minus_1(sa):
    x = cases.points(3, 2)
    idx, dist = sa.nearest_neighbors(x, 5, "euclidean")
    assert idx.shape == (3, 2)
    with sa.fuzzy_simplicial_set(idx, dist) as want, sa.umap_graph(x, 5, "euclidean") as g:
        assert g.k == 2
        same(outputs(g, 200.0), outputs(want, 200.0), "n = 3, k = 5")
    with pytest.raises(sa.ScanrsError, match="no rows or no columns"):
        sa.umap_graph(x[:1], 5, "euclidean")


N_FILTER = 4096  # the smallest shape of the filtered search, as tests/test_gpu_metric_knn.py sets it up


@pytest.mark.parametrize("kind", KINDS)
def test_umap_graph_equals_the_graph_of_nearest_neighbors_filtered(sa, kind):
    x = knn_cases.clustered_points(N_FILTER, 50)
    with options(sa, min_points=1024):
        idx, dist = sa.nearest_neighbors(x, 15, kind)
        filtered = sa.debug_knn_last_stats()["filtered"]
        assert filtered or kind == "euclidean"
        with sa.fuzzy_simplicial_set(idx, dist) as want, sa.umap_graph(x, 15, kind) as g:
            assert sa.debug_knn_last_stats()["filtered"] == filtered
            same(outputs(g, 200.0), outputs(want, 200.0), (kind, "filtered"))
    with sa.host_fuzzy_simplicial_set(idx, dist) as twin, sa.fuzzy_simplicial_set(idx, dist) as g:
        same(outputs(g, 200.0), outputs(twin, 200.0), (kind, "4096 rows against the twin"))


def test_the_star_and_the_widest_staging(sa):
    idx, dist = cases.star()
    with sa.host_fuzzy_simplicial_set(idx, dist) as twin, sa.fuzzy_simplicial_set(idx, dist) as g:
        indptr = g.to_csr()[0]
        assert int(indptr[1]) - int(indptr[0]) == 1499  # row 0 is named by every other row
        same(outputs(g, 500.0), outputs(twin, 500.0), "star")
    idx, dist = cases.lists(sa, 257, 10, 128)  # 64 x 129 doubles of LDS per wave, four full waves and one with a single row
    for lc in (1.0, 3.25):
        with sa.host_fuzzy_simplicial_set(idx, dist, local_connectivity=lc) as twin, sa.fuzzy_simplicial_set(idx, dist, local_connectivity=lc) as g:
            same(outputs(g, 200.0), outputs(twin, 200.0), ("k = 128", lc))


def test_a_repeat_run_gives_identical_bits(sa):
    idx, dist = cases.lists(sa, 1000, 10, 15)
    runs = []
    for _ in range(3):
        with sa.fuzzy_simplicial_set(idx, dist, set_op_mix_ratio=0.5) as g:
            runs.append(outputs(g, 200.0))
    same(runs[1], runs[0], "second run")
    same(runs[2], runs[0], "third run")


def test_the_refusals_and_the_memory_they_leave(sa):
    before = in_use(sa)
    for name, idx, dist, kw, text in cases.refusal_cases():
        if idx.size == 0:
            with pytest.raises(sa.ScanrsError, match=text):
                sa.fuzzy_simplicial_set(np.zeros(idx.shape, np.uint32), np.zeros(idx.shape), **kw)
        else:
            with pytest.raises(sa.ScanrsError) as e:
                sa.fuzzy_simplicial_set(idx, dist, **kw)
            assert e.value.code == 6 and text in str(e.value), (name, str(e.value))
            with pytest.raises(sa.ScanrsError) as e_twin:
                sa.host_fuzzy_simplicial_set(idx, dist, **kw)
            assert str(e.value) == str(e_twin.value), name
            ti, td = device_lists(np.ascontiguousarray(idx, np.uint32), np.ascontiguousarray(dist, np.float64), idx.shape[1])
            with pytest.raises(sa.ScanrsError) as e_dev:
                sa.fuzzy_simplicial_set_device(ti.data_ptr(), td.data_ptr(), idx.shape[0], idx.shape[1], idx.shape[1], **kw)
            assert str(e.value) == str(e_dev.value), name
        assert in_use(sa) == before, name
    idx, dist = cases.padded()
    ti, td = device_lists(idx, dist, 5)
    with pytest.raises(sa.ScanrsError, match="leading dimension"):
        sa.fuzzy_simplicial_set_device(ti.data_ptr(), td.data_ptr(), 3, 4, 5)
    x = cases.points(65, 2)
    x[7, 1] = np.inf
    with pytest.raises(sa.ScanrsError, match="row 7 "):
        sa.umap_graph(x, 5, "cosine")
    with pytest.raises(sa.ScanrsError, match="local_connectivity"):
        sa.umap_graph(cases.points(65, 2), 5, "cosine", local_connectivity=-1.0)
    assert in_use(sa) == before
    with sa.fuzzy_simplicial_set(idx, dist) as g:
        assert in_use(sa) > before
        for bad in (0.0, -3.0, np.nan):
            with pytest.raises(sa.ScanrsError, match="n_epochs"):
                g.edges(bad)
    assert in_use(sa) == before
