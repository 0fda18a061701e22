"""merge_clusters on the device (scan-rs_amd/csrc/cluster.hip, cluster_host.cpp) against the CPU restatement tests/merge_ref.py:
the medoids against a sort, the merge's labels and candidate trace against the reference's loop, both copies of the matrix, the
fused route against the literal one, and the refusals."""
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


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd
    import scanrs_amd.hdf5_io  # noqa: F401

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


def _golden(name):
    return os.path.join(TESTS, "golden", name)


def _handle(sa, m, storage):
    """genes x cells scipy matrix -> handle in the given storage (CSR: gene-major, CSC: cell-major)."""
    g, c = m.shape
    s = sparse.csr_matrix(m) if storage == sa.CSR else sparse.csc_matrix(m)
    s.sort_indices()
    return sa.AdaptiveMat.from_csmat(g, c, storage, s.indptr.astype(np.uint64), s.indices.astype(np.uint32), s.data.astype(np.uint32))


def _planted(sizes, splits, genes, d, seed, marker_genes=30, effect=4.0):
    """Populations with their own expression profile (marker genes up by `effect`) and their own score centre; population p is
    cut into splits[p] labels along its first score coordinate. Returns (genes x cells CSR u32, cells x d scores, labels)."""
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    pop = np.repeat(np.arange(len(sizes)), sizes)
    base = rng.gamma(0.6, 0.5, genes)
    prof = np.tile(base, (len(sizes), 1))
    for p in range(len(sizes)):
        prof[p, rng.choice(genes, marker_genes, replace=False)] *= effect
    lib = rng.lognormal(0.0, 0.3, n)
    counts = rng.poisson(prof[pop].T * lib).astype(np.uint32)  # genes x cells
    centres = rng.standard_normal((len(sizes), d)) * 8.0
    scores = centres[pop] + rng.standard_normal((n, d))
    labels = np.zeros(n, dtype=np.int64)
    nxt = 0
    for p, k in enumerate(splits):
        idx = np.flatnonzero(pop == p)
        order = idx[np.argsort(scores[idx, 0], kind="stable")]
        for j, part in enumerate(np.array_split(order, k)):
            labels[part] = nxt + j
        nxt += k
    relabel = rng.permutation(nxt)  # label numbers unrelated to the populations
    return sparse.csr_matrix(counts), scores, relabel[labels].astype(np.int16)


@pytest.fixture(scope="module")
def planted():
    # 4 populations cut into 9 labels, plus one distinct population: 10 labels
    return _planted([800, 700, 600, 500, 400], [3, 2, 2, 2, 1], 500, 6, 3)


def _assert_trace(tr, exp, rtol=1e-6):
    got = [(a, b, c) for a, b, c, _ in tr.entries]
    assert got == [(a, b, c) for a, b, c, _ in exp["entries"]]
    np.testing.assert_allclose([p for *_, p in tr.entries], [p for *_, p in exp["entries"]], rtol=rtol, atol=0)
    assert (tr.n_candidates, tr.n_rounds, tr.n_merges) == (exp["n_candidates"], exp["n_rounds"], exp["n_merges"])


def _same_trace_bits(t1, t2):
    for f in ("leaf0", "leaf1", "n_de", "min_p_adj"):
        assert getattr(t1, f).tobytes() == getattr(t2, f).tobytes(), f
    assert (t1.n_candidates, t1.n_rounds, t1.n_merges) == (t2.n_candidates, t2.n_rounds, t2.n_merges)


# ---- 1. medoids ---------------------------------------------------------------------------------------------------------------
def _expected_medoids(x, labels, k):
    out = np.zeros((k, x.shape[1]))
    for i in range(k):
        rows = x[labels == i]
        for c in range(x.shape[1]):
            out[i, c] = mref.median_mut(list(rows[:, c]))
            assert out[i, c] == np.median(rows[:, c])
    return out


def _device_scores(x, ld):
    import torch

    t = torch.zeros((x.shape[0], ld), dtype=torch.float64, device="cuda")
    t[:, : x.shape[1]] = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    return t


def test_medoids_odd_even_singletons_ties_and_signed_zeros(sa):
    rng = np.random.default_rng(1)
    sizes = [1, 2, 3, 4, 7, 10, 1, 64, 65, 500, 1001]
    labels = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(labels)
    n, d = len(labels), 7
    x = rng.standard_normal((n, d))
    x[:, 1] = np.round(x[:, 1])  # repeated values
    x[:, 2] = rng.choice([-0.0, 0.0, 1.0, -1.0], n)  # signed zeros
    x[:, 3] = rng.choice([-1e300, 1e-300, -5e-324, 3.0], n)
    exp = _expected_medoids(x, labels, len(sizes))
    got = sa.medioids(x, labels)
    np.testing.assert_array_equal(got, exp)  # == (±0.0 compare equal)
    # device form with a leading dimension above d
    t = _device_scores(x, 11)
    dev = sa.PcaResultDevice(0, 0, t.data_ptr(), 11, d, 0, n)
    got_d = sa.medioids(dev, labels)
    assert got_d.tobytes() == got.tobytes()
    assert sa.medioids(x, labels).tobytes() == got.tobytes()  # independent of launch timing


@pytest.mark.parametrize("k", [1, 8192])
def test_medoids_k_extremes(sa, k):
    rng = np.random.default_rng(k)
    n = max(5000, 3 * k)
    labels = np.concatenate([np.arange(k), rng.integers(0, k, n - k)])
    rng.shuffle(labels)
    x = np.round(rng.standard_normal((n, 4)), 2)
    got = sa.medioids(x, labels)
    exp = np.zeros((k, 4))
    order = np.argsort(labels, kind="stable")
    bounds = np.searchsorted(labels[order], np.arange(k + 1))
    for i in range(k):
        rows = x[order[bounds[i]:bounds[i + 1]]]
        exp[i] = np.median(rows, axis=0)
    np.testing.assert_array_equal(got, exp)
    t = _device_scores(x, 4)
    assert sa.medioids(sa.PcaResultDevice(0, 0, t.data_ptr(), 4, 4, 0, n), labels).tobytes() == got.tobytes()


def test_medoids_refuse_bad_labels_and_nan(sa):
    x = np.zeros((6, 2))
    with pytest.raises(sa.ScanrsError, match="label 2 has no cell"):
        sa.medioids(x, [0, 1, 3, 0, 1, 3])
    with pytest.raises(sa.ScanrsError, match="cell 1"):
        sa.medioids(x, [0, -1, 0, 0, 0, 0])
    x[4, 1] = np.nan
    with pytest.raises(sa.ScanrsError, match="cell 4"):
        sa.medioids(x, [0, 0, 0, 0, 0, 0])


# ---- 2. merge_clusters against the restatement -------------------------------------------------------------------------------------
def test_merge_planted_matches_restatement(sa, planted):
    m, x, labels = planted
    exp_labels, exp = mref.merge_clusters(m, x, labels)
    assert exp["n_merges"] > 0 and exp["n_candidates"] > exp["n_merges"]  # the fixture exercises both outcomes
    got, tr = sa.merge_clusters(_handle(sa, m, sa.CSR), x, labels, trace=True)
    np.testing.assert_array_equal(got, exp_labels)
    _assert_trace(tr, exp)
    assert tr.n_passes == 2  # totals + one grouped pass


def test_merge_orientations_give_the_same_bits(sa, planted):
    m, x, labels = planted
    l1, t1 = sa.merge_clusters(_handle(sa, m, sa.CSR), x, labels, trace=True)
    l2, t2 = sa.merge_clusters(_handle(sa, m, sa.CSC), x, labels, trace=True)
    np.testing.assert_array_equal(l1, l2)
    _same_trace_bits(t1, t2)
    # two calls give identical bits
    l3, t3 = sa.merge_clusters(_handle(sa, m, sa.CSC), x, labels, trace=True)
    np.testing.assert_array_equal(l2, l3)
    _same_trace_bits(t2, t3)


def test_merge_on_tiny_10x_graphclust(sa):
    h5 = sa.hdf5_io.read_csc_matrix(_golden("tiny_10x.h5"))
    m = sparse.csc_matrix((h5.values, h5.indices, h5.indptr.astype(np.int64)), shape=(h5.rows, h5.cols))
    nc, clusters = sa.hdf5_io.get_clustering(_golden("tiny_analysis.h5"), "_graphclust")
    labels = sa.labels_from_clustering(clusters)
    assert labels.min() == 0 and len(np.unique(labels)) == nc
    h = _handle(sa, m, sa.CSC)
    nh = sa.normalize(h, sa.Normalization.CellRanger)
    _, _, v = sa.BkSvd().run_pca(nh, 10)
    exp_labels, exp = mref.merge_clusters(m, v, labels)
    got, tr = sa.merge_clusters(h, v, labels, trace=True)
    np.testing.assert_array_equal(got, exp_labels)
    _assert_trace(tr, exp)
    # the scores straight from the PCA's device copy
    got_d, tr_d = sa.merge_clusters(h, sa.pca_result_device(nh), labels, trace=True)
    np.testing.assert_array_equal(got_d, got)
    _same_trace_bits(tr, tr_d)


# ---- 3. fused route against the literal one ------------------------------------------------------------------------------------------
def test_fused_against_literal_at_100k_cells(sa):
    m, x, labels = _planted([30000, 25000, 20000, 15000, 10000], [3, 2, 2, 2, 1], 300, 8, 5)
    h = _handle(sa, m, sa.CSC)
    lf, tf = sa.merge_clusters(h, x, labels, trace=True)
    h.set_option("merge_fused", 0)
    ll, tl = sa.merge_clusters(h, x, labels, trace=True)
    np.testing.assert_array_equal(lf, ll)
    assert [e[:3] for e in tf.entries] == [e[:3] for e in tl.entries]
    np.testing.assert_allclose(tf.min_p_adj, tl.min_p_adj, rtol=1e-6, atol=0)
    assert tf.n_merges > 0
    assert tf.n_passes == 2 and tl.n_passes == 4 * tl.n_candidates


# ---- 4. edge cases --------------------------------------------------------------------------------------------------------------------
def test_union_with_median_total_zero_takes_the_literal_route(sa):
    # clusters 0 and 1 are mostly empty cells: their union's median total is 0 and the size factors are not finite
    rng = np.random.default_rng(7)
    genes = 40
    sizes = [30, 30, 40]
    n = sum(sizes)
    labels = np.repeat(np.arange(3), sizes).astype(np.int16)
    counts = rng.poisson(2.0, (genes, n)).astype(np.uint32)
    counts[:, :25] = 0
    counts[:, 30:55] = 0
    x = np.concatenate([rng.standard_normal((30, 2)), rng.standard_normal((30, 2)) + 0.5, rng.standard_normal((40, 2)) + 30.0])
    m = sparse.csr_matrix(counts)
    h = _handle(sa, m, sa.CSR)
    lf, tf = sa.merge_clusters(h, x, labels, trace=True)
    assert (tf.leaf0[0], tf.leaf1[0]) == (0, 1)
    h.set_option("merge_fused", 0)
    ll, tl = sa.merge_clusters(h, x, labels, trace=True)
    np.testing.assert_array_equal(lf, ll)
    # the first candidate ran the literal route in both: the same bits; later unions have a median total above 0
    assert tf.entries[0][:3] == tl.entries[0][:3]
    assert tf.min_p_adj[:1].tobytes() == tl.min_p_adj[:1].tobytes()
    assert [e[:3] for e in tf.entries] == [e[:3] for e in tl.entries]
    np.testing.assert_allclose(tf.min_p_adj, tl.min_p_adj, rtol=1e-6, atol=0)


def test_small_cases(sa):
    m = sparse.csr_matrix(np.random.default_rng(2).poisson(1.0, (20, 12)).astype(np.uint32))
    x = np.random.default_rng(3).standard_normal((12, 3))
    h = _handle(sa, m, sa.CSR)
    got, tr = sa.merge_clusters(h, x, np.zeros(12, dtype=np.int16), trace=True)
    np.testing.assert_array_equal(got, np.zeros(12))
    assert (tr.n_candidates, tr.n_rounds, tr.n_merges) == (0, 1, 0)
    two = (np.arange(12) % 2).astype(np.int16)
    exp_labels, exp = mref.merge_clusters(m, x, two)
    got, tr = sa.merge_clusters(h, x, two, trace=True)
    np.testing.assert_array_equal(got, exp_labels)
    _assert_trace(tr, exp)
    empty = _handle(sa, sparse.csr_matrix((20, 0), dtype=np.uint32), sa.CSR)
    assert sa.merge_clusters(empty, np.zeros((0, 3)), np.zeros(0, dtype=np.int16)).shape == (0,)


def test_refusals(sa, planted):
    m, x, labels = planted
    h = _handle(sa, m, sa.CSR)
    bad = labels.copy()
    bad[bad == 3] = 4  # label 3 missing
    with pytest.raises(sa.ScanrsError, match="label 3 has no cell"):
        sa.merge_clusters(h, x, bad)
    bad = labels.copy()
    bad[17] = -1
    with pytest.raises(sa.ScanrsError, match="cell 17"):
        sa.merge_clusters(h, x, bad)
    xn = x.copy()
    xn[5, 2] = np.nan
    with pytest.raises(sa.ScanrsError, match="cell 5"):
        sa.merge_clusters(h, xn, labels)
    with pytest.raises(sa.ScanrsError):
        sa.merge_clusters(h, x, labels[:-1])
    with pytest.raises(sa.ScanrsError):
        sa.merge_clusters(h, x[:-1], labels)
    hs = _handle(sa, m, sa.CSC)
    hs.set_shard(0, 1, 0, m.shape[1], lambda *a: 0)
    with pytest.raises(sa.ScanrsError, match="sharded"):
        sa.merge_clusters(hs, x, labels)


def test_cancel(sa, planted):
    m, x, labels = planted
    sn = sa.AtomicSnoop()
    sn.cancel()
    with pytest.raises(sa.CancellationError) as e:
        sa.merge_clusters(_handle(sa, m, sa.CSR), x, labels, snoop=sn)
    assert e.value.code == 3


def test_many_clusters_tile_the_gene_major_pass(sa):
    # 1600 clusters > 1536 per gene-major tile: two tiles against the cell-major copy's single scatter pass. Cluster j expresses
    # gene j alone; with 3 cells a side, some pairs still have no DE gene and merge.
    k, per = 1600, 3
    rng = np.random.default_rng(11)
    n = k * per
    labels = np.repeat(np.arange(k), per).astype(np.int16)
    counts = sparse.lil_matrix((k + 20, n), dtype=np.uint32)
    for j in range(k):
        counts[j, j * per:(j + 1) * per] = 60
    counts = sparse.csr_matrix(counts) + sparse.random(k + 20, n, density=0.01, format="csr", random_state=3,
                                                       data_rvs=lambda s: rng.integers(1, 4, s)).astype(np.uint32)
    x = np.repeat(rng.standard_normal((k, 4)) * 10, per, axis=0) + rng.standard_normal((n, 4)) * 0.01
    l1, t1 = sa.merge_clusters(_handle(sa, counts, sa.CSR), x, labels, trace=True)
    l2, t2 = sa.merge_clusters(_handle(sa, counts, sa.CSC), x, labels, trace=True)
    assert t1.n_passes == 3 and t2.n_passes == 2  # totals + two tiles / totals + one scatter pass
    assert t1.n_candidates > 100 and t1.n_candidates > t1.n_merges
    np.testing.assert_array_equal(l1, l2)
    _same_trace_bits(t1, t2)
