"""merge_clusters and the cluster medoids over sharded and multi-GPU matrices: centres, labels and every trace field
from a `MultiMat` or a sharded handle must equal the call on one unsharded `AdaptiveMat` bit for bit, for any number of shards. The
fixtures are tests/merge_sharded_case.py; the references are computed once per module."""
import os
import sys

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import merge_ref as mref  # noqa: E402
import merge_sharded_case as mc  # noqa: E402

FORMS = ("csc", "csr_t")


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


def _handle(sa, m, storage="csc"):
    s = sparse.csc_matrix(m) if storage == "csc" else sparse.csr_matrix(m)
    s.sort_indices()
    return sa.AdaptiveMat.from_csmat(s.shape[0], s.shape[1], sa.CSC if storage == "csc" else sa.CSR, s.indptr.astype(np.uint64),
                                     s.indices.astype(np.uint32), s.data.astype(np.uint32))


def _multi(sa, m, form, n_shards):
    """genes x cells scipy matrix -> (MultiMat with the cells sharded, transposed flag)."""
    s = sparse.csc_matrix(m)
    s.sort_indices()
    g, c = s.shape
    ip, ix, vv = s.indptr.astype(np.uint64), s.indices.astype(np.uint32), s.data.astype(np.uint32)
    if form == "csc":
        return sa.MultiMat(g, c, sa.CSC, ip, ix, vv, n_shards, devices=[0] * n_shards), False
    return sa.MultiMat(c, g, sa.CSR, ip, ix, vv, n_shards, devices=[0] * n_shards), True


def _device_scores(x, ld):
    import torch

    t = torch.zeros((x.shape[0], ld), dtype=torch.float64, device="cuda")
    t[:, : x.shape[1]] = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    return t


def _same_trace_bits(t1, t2):
    for f in ("leaf0", "leaf1", "n_de", "min_p_adj"):
        assert getattr(t1, f).tobytes() == getattr(t2, f).tobytes(), f
    assert (t1.n_candidates, t1.n_rounds, t1.n_merges) == (t2.n_candidates, t2.n_rounds, t2.n_merges)


# ---- 1. medoids --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def medoid_case(sa):
    m, x, labels = mc.medoid_case()
    exp = sa.medioids(x, labels)
    k = len(mc.MEDOID_SIZES)
    for i in range(k):  # the unsharded centres are the sorted lists' medians
        for c in range(x.shape[1]):
            assert exp[i, c] == mref.median_mut(list(x[labels == i][:, c]))
    return m, x, labels, exp


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_shards", mc.SHARDS)
def test_medoids_equal_the_unsharded_centres_bit_for_bit(sa, medoid_case, n_shards, form):
    m, x, labels, exp = medoid_case
    mm, transposed = _multi(sa, m, form, n_shards)
    ranges = mm.shard_ranges()
    assert ranges[0][2] >= 255  # cluster 2 lies inside the first shard
    if n_shards > 1:  # the two cells of cluster 1 - its two middle elements - lie in different shards
        owner = [next(i for i, (_, lo, hi) in enumerate(ranges) if lo <= c < hi) for c in mc.MEDOID_PAIR]
        assert owner[0] != owner[1]
    got = sa.cluster_medoids(mm, x, labels, transposed=transposed)
    assert got.tobytes() == exp.tobytes()
    # 8 radix rounds of one (cluster, column) tile, and the NaN slots
    assert [mm.counter("de_shard_allreduces", i) for i in range(n_shards)] == [9] * n_shards
    assert sa.cluster_medoids(mm, x, labels, n_clusters=len(mc.MEDOID_SIZES), transposed=transposed).tobytes() == exp.tobytes()
    mm.close()


def test_medoids_name_the_first_nan_cell_and_refuse_bad_labels(sa, medoid_case):
    m, x, labels, _ = medoid_case
    xn = x.copy()
    xn[1200, 3] = np.nan
    xn[411, 5] = np.nan
    xn[412, 0] = np.nan
    with pytest.raises(sa.ScanrsError) as plain:
        sa.medioids(xn, labels)
    assert "the scores of cell 411 hold a NaN" in str(plain.value)
    for n_shards in (2, 5):
        mm, _ = _multi(sa, m, "csc", n_shards)
        with pytest.raises(sa.ScanrsError) as e:
            sa.cluster_medoids(mm, xn, labels)
        assert e.value.code == 6 and "the scores of cell 411 hold a NaN" in str(e.value)
        bad = labels.copy()
        bad[bad == 0] = 5  # label 0 missing
        with pytest.raises(sa.ScanrsError, match="label 0 has no cell"):
            sa.cluster_medoids(mm, x, bad)
        with pytest.raises(sa.ScanrsError):
            sa.cluster_medoids(mm, x, labels[:-1])
        with pytest.raises(sa.ScanrsError):
            sa.cluster_medoids(mm, x[:-1], labels)
        assert sa.cluster_medoids(mm, x, labels).tobytes() == sa.medioids(x, labels).tobytes()  # the handle serves the next call
        mm.close()


def test_medoids_through_a_host_hook_and_device_scores(sa, medoid_case):
    m, x, labels, exp = medoid_case
    calls = []

    def hook(ptr, count, dtype):
        calls.append((count, dtype))
        return 0

    h = _handle(sa, m)
    h.set_shard(0, 1, 0, m.shape[1], hook)
    assert sa.cluster_medoids_sharded(h, x, labels).tobytes() == exp.tobytes()
    pairs = len(mc.MEDOID_SIZES) * mc.MEDOID_D
    assert calls == [(pairs * 512, 1)] * 8 + [(1, 1)]
    t = _device_scores(x, 9)  # the rank's own cells in device memory, a leading dimension above d
    dev = sa.PcaResultDevice(0, 0, t.data_ptr(), 9, mc.MEDOID_D, 0, m.shape[1])
    assert sa.cluster_medoids_sharded(h, dev, labels).tobytes() == exp.tobytes()
    assert sa.cluster_medoids_sharded(_handle(sa, m), x, labels).tobytes() == exp.tobytes()  # an unsharded handle: the plain call
    assert sa.cluster_medoids(_handle(sa, m), x, labels).tobytes() == exp.tobytes()


# ---- 2. merge_clusters ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(sa):
    m, x, labels = mc.planted_default()
    exp_labels, exp = mref.merge_clusters(m, x, labels)
    assert exp["n_merges"] > 0 and exp["n_candidates"] > exp["n_merges"]  # the fixture exercises both outcomes
    h = _handle(sa, m)
    ref = {}
    for fused in (1, 0):
        h.set_option("merge_fused", fused)
        ref[fused] = sa.merge_clusters(h, x, labels, trace=True)
    return dict(m=m, x=x, labels=labels, exp_labels=exp_labels, exp=exp, ref=ref)


def _assert_trace(tr, exp, rtol=1e-6):  # tests/test_gpu_merge_clusters.py::_assert_trace
    got = [(a, b, c) for a, b, c, _ in tr.entries]
    assert got == [(a, b, c) for a, b, c, _ in exp["entries"]]
    np.testing.assert_allclose([p for *_, p in tr.entries], [p for *_, p in exp["entries"]], rtol=rtol, atol=0)
    assert (tr.n_candidates, tr.n_rounds, tr.n_merges) == (exp["n_candidates"], exp["n_rounds"], exp["n_merges"])


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("n_shards", [1, 2, 3])
def test_merge_equals_the_unsharded_call_bit_for_bit(sa, planted, n_shards, fused):
    form = FORMS[(n_shards + fused) % 2]  # both forms occur with both routes
    mm, transposed = _multi(sa, planted["m"], form, n_shards)
    mm.set_option("merge_fused", fused)
    got, tr = sa.merge_clusters(mm, planted["x"], planted["labels"], trace=True, transposed=transposed)  # scores: the global host array
    ref_labels, ref_tr = planted["ref"][fused]
    assert got.tobytes() == ref_labels.tobytes()
    _same_trace_bits(tr, ref_tr)
    assert tr.n_passes == ref_tr.n_passes
    np.testing.assert_array_equal(got, planted["exp_labels"])
    _assert_trace(tr, planted["exp"])
    steps = [mm.counter("de_shard_allreduces", i) for i in range(n_shards)]
    tests = [mm.counter("de_shard_tests", i) for i in range(n_shards)]
    assert len(set(steps)) == 1 and min(tests) > 0
    if fused:
        # totals and one accumulator tile; per round 8 radix rounds of one tile + the NaN slots; one gather of p-values per candidate
        assert steps[0] == 2 + 9 * tr.n_rounds + tr.n_candidates
    else:
        assert steps[0] == 9 * tr.n_rounds + 5 * tr.n_candidates  # §7g's 3 + 2 per candidate
    mm.close()


def test_merge_with_the_cells_shuffled_over_the_shards(sa):
    m, x, labels = mc.planted_shuffled()
    ref_labels, ref_tr = sa.merge_clusters(_handle(sa, m), x, labels, trace=True)
    mm, transposed = _multi(sa, m, "csc", 3)
    got, tr = sa.merge_clusters(mm, x, labels, trace=True, transposed=transposed)
    assert got.tobytes() == ref_labels.tobytes()
    _same_trace_bits(tr, ref_tr)
    mm.close()


def test_merge_on_one_handle_with_a_host_hook_and_device_scores(sa, planted):
    m, x, labels = planted["m"], planted["x"], planted["labels"]
    calls = []

    def hook(ptr, count, dtype):
        calls.append((count, dtype))
        return 0

    h = _handle(sa, m)
    h.set_shard(0, 1, 0, m.shape[1], hook)
    ref_labels, ref_tr = planted["ref"][1]
    got, tr = sa.merge_clusters_sharded(h, x, labels, trace=True)
    assert got.tobytes() == ref_labels.tobytes()
    _same_trace_bits(tr, ref_tr)
    assert calls and {d for _, d in calls} == {1} and len(calls) == h.counter("de_shard_allreduces")
    t = _device_scores(x, 8)  # pca_is_device = 1: the rank's own cells
    dev = sa.PcaResultDevice(0, 0, t.data_ptr(), 8, x.shape[1], 0, m.shape[1])
    got, tr = sa.merge_clusters_sharded(h, dev, labels, trace=True)
    assert got.tobytes() == ref_labels.tobytes()
    _same_trace_bits(tr, ref_tr)
    got, tr = sa.merge_clusters_sharded(_handle(sa, m, "csr"), x, labels, trace=True)  # an unsharded handle: the plain call
    assert got.tobytes() == ref_labels.tobytes()
    _same_trace_bits(tr, ref_tr)


# ---- 3. cancellation and refusals -----------------------------------------------------------------------------------------------------------
def test_cancel_and_refusals(sa, planted):
    m, x, labels = planted["m"], planted["x"], planted["labels"]
    mm, transposed = _multi(sa, m, "csc", 2)
    sn = sa.AtomicSnoop()
    sn.cancel()
    with pytest.raises(sa.CancellationError) as e:
        sa.merge_clusters(mm, x, labels, snoop=sn, transposed=transposed)
    assert e.value.code == 3
    for kw in (dict(labels=labels[:-1]), dict(pca=x[:-1])):
        with pytest.raises(sa.ScanrsError):
            sa.merge_clusters(mm, **{"pca": x, "labels": labels, **kw})
    bad = labels.copy()
    bad[17] = -1
    with pytest.raises(sa.ScanrsError, match="cell 17"):
        sa.merge_clusters(mm, x, bad)
    got = sa.merge_clusters(mm, x, labels, transposed=transposed)  # the handle serves the next call
    assert got.tobytes() == planted["ref"][1][0].tobytes()
    mm.close()
    # the genes sharded
    s = sparse.csr_matrix(m)
    s.sort_indices()
    ip, ix, vv = s.indptr.astype(np.uint64), s.indices.astype(np.uint32), s.data.astype(np.uint32)
    mg = sa.MultiMat(m.shape[0], m.shape[1], sa.CSR, ip, ix, vv, 2, devices=[0, 0])
    hg = sa.AdaptiveMat.from_csmat(m.shape[0], m.shape[1], sa.CSR, ip, ix, vv)
    hg.set_shard(0, 1, 0, m.shape[0], lambda *a: 0)
    for call in (lambda: sa.merge_clusters(mg, x, labels), lambda: sa.cluster_medoids(mg, x, labels), lambda: sa.merge_clusters_sharded(hg, x, labels)):
        with pytest.raises(sa.ScanrsError) as e:
            call()
        assert e.value.code == 6 and "cells" in str(e.value) and "sharded" in str(e.value)
    mg.close()
    # the plain entry points keep refusing a sharded AdaptiveMat
    hs = _handle(sa, m)
    hs.set_shard(0, 1, 0, m.shape[1], lambda *a: 0)
    with pytest.raises(sa.ScanrsError, match="sharded"):
        sa.merge_clusters(hs, x, labels)
    with pytest.raises(sa.ScanrsError, match="sharded"):
        sa.sseq_de_pairs(hs, labels, [(1, 0)])
