"""kNN over sharded and multi-GPU score matrices (nn.rs:38-83) against `knn` of the whole point set on one device:
the indices must be EQUAL (np.array_equal), whatever the shard cut and the block size, and the squared distances must carry the
bits of the library's fma chain recomputed for the returned indices (tests/knn_sharded_ref.py). Where the coordinates are small
integers the result is also compared with the restatement of the reference's oracle (oracle/knn_oracle.py). All shards share device 0.

Two forms: a MultiMat (the library cuts the cells and drives the shards), and handles bound with set_shard to explicit cuts, one
thread per rank, with a host hook that sums the ranks' buffers and records the dtypes it saw."""
import contextlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
for p in (TESTS, os.path.join(os.path.dirname(TESTS), "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import knn_oracle  # noqa: E402
import knn_sharded_ref as ref  # noqa: E402
from shard_ring import Ring, run_ranks  # noqa: E402

DEFAULT_BLOCK_ROWS = 262144
U32MAX = ref.U32MAX


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


@contextlib.contextmanager
def options(sa, block_rows=DEFAULT_BLOCK_ROWS, min_points=32768):
    sa.set_global_option("knn_block_rows", block_rows)
    sa.set_global_option("knn_filter_min_points", min_points)
    try:
        yield
    finally:
        sa.set_global_option("knn_block_rows", DEFAULT_BLOCK_ROWS)
        sa.set_global_option("knn_filter_min_points", 32768)


def whole(sa, pts, k):
    """`knn` of the whole point set on one device, by the exhaustive kernel (the reference of every case)."""
    sa.set_global_option("knn_exhaustive", 1)
    try:
        return sa.knn(pts, k)
    finally:
        sa.set_global_option("knn_exhaustive", 0)


def oracle(pts, k):
    return knn_oracle.exhaustive_find_nn(pts, pts, k, include_self=False).astype(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), int(np.sum(a.view(np.uint64) != b.view(np.uint64)))


def check(sa, pts, k, got, dist, want):
    assert got.dtype == np.uint32 and got.shape == want.shape
    assert np.array_equal(got, want), f"{int(np.sum(np.any(got != want, axis=1)))} rows differ"
    same_bits(dist, ref.sq_dist_pairs(pts, got))
    d, i = dist, got.astype(np.int64)
    assert np.all((np.diff(d, axis=1) > 0) | ((np.diff(d, axis=1) == 0) & (np.diff(i, axis=1) > 0)) | (i[:, 1:] == U32MAX))
    assert not np.any(got == np.arange(len(pts), dtype=np.uint32)[:, None])  # a query's own row never appears


def cell_matrix(n_cells):
    """a genes x cells CSC matrix with one count per cell: the handle only gives the transport and the range of cells"""
    return np.arange(n_cells + 1, dtype=np.uint64), np.zeros(n_cells, dtype=np.uint32), np.ones(n_cells, dtype=np.uint32)


class Hooked:
    """Handles bound with set_shard to explicit cuts, one thread per rank."""

    def __init__(self, sa, cuts):
        self.sa, self.cuts, self.world = sa, list(cuts), len(cuts) - 1
        self.ring = Ring(self.world)
        self.hs = []
        for r, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            h = sa.AdaptiveMat.from_csmat(1, hi - lo, sa.CSC, *cell_matrix(hi - lo))
            h.set_shard(r, self.world, lo, cuts[-1], self.ring.hook(r))
            self.hs.append(h)

    def on_all(self, fn):
        """[result or exception] per rank"""
        out, err = run_ranks(self.world, lambda r: fn(r, self.hs[r]))
        return [o if e is None else e for o, e in zip(out, err)]

    def knn(self, pts, k, per_rank_k=None):
        out = self.on_all(lambda r, h: h.knn_sharded(pts, per_rank_k[r] if per_rank_k else k, return_sq_dist=True))
        for o in out:
            if isinstance(o, BaseException):
                raise o
        return np.concatenate([o[0] for o in out], axis=0), np.concatenate([o[1] for o in out], axis=0)

    def counters(self, key):
        return [h.counter(key) for h in self.hs]

    def close(self):
        pass


class Multi:
    """A MultiMat with all shards on device 0 (the library cuts the cells)."""

    def __init__(self, sa, n, world):
        self.world = world
        self.mm = sa.MultiMat(1, n, sa.CSC, *cell_matrix(n), world, devices=[0] * world)

    def knn(self, pts, k):
        return self.mm.knn(k, pts, return_sq_dist=True)

    def counters(self, key):
        return [self.mm.counter(key, shard=i) for i in range(self.world)]

    def close(self):
        self.mm.close()


def make(sa, form, n, cuts):
    return Multi(sa, n, len(cuts) - 1) if form == "multi" else Hooked(sa, cuts)


FORMS = ("multi", "hook")


# ---- 1. the exhaustive route on the lattice ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice(sa):
    pts = ref.lattice_points()
    want = {k: whole(sa, pts, k) for k in ref.LATTICE_K}
    for k in ref.LATTICE_K:
        assert np.array_equal(want[k], oracle(pts, k))
    return pts, want


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("block_rows", ref.LATTICE_BLOCKS)
@pytest.mark.parametrize("shards", sorted(ref.LATTICE_CUTS))
def test_lattice_with_ties_and_duplicates(sa, lattice, shards, block_rows, form):
    pts, want = lattice
    cuts = ref.LATTICE_CUTS[shards]
    run = make(sa, form, ref.LATTICE_N, cuts)
    try:
        with options(sa, block_rows=block_rows):
            for k in ref.LATTICE_K:
                got, dist = run.knn(pts, k)
                check(sa, pts, k, got, dist, want[k])
                assert np.array_equal(got, oracle(pts, k))
                n_blocks = len(ref.block_plan(ref.LATTICE_N, block_rows))
                assert run.counters("knn_blocks") == [n_blocks] * shards
                assert run.counters("knn_allreduces") == [n_blocks + 1] * shards
                assert not sa.debug_knn_last_stats()["filtered"]
        if form == "hook":
            assert run.ring.dtypes == {1}  # 8. only integers cross the shards
    finally:
        run.close()


# ---- 2. padding ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_padding_when_fewer_than_k_other_points_exist(sa, form):
    pts, k, n = ref.padding_points(), ref.PADDING_K, ref.PADDING_N
    run = make(sa, form, n, ref.PADDING_CUTS)
    try:
        with options(sa, block_rows=4):
            got, dist = run.knn(pts, k)
    finally:
        run.close()
    assert np.array_equal(got, oracle(pts, k)) and np.array_equal(got, sa.find_nn(pts, k, pts, False))
    assert np.all(got[:, n - 1:] == U32MAX) and np.all(np.isposinf(dist[:, n - 1:])) and np.all(got[:, : n - 1] < n)
    same_bits(dist, ref.sq_dist_pairs(pts, got))
    for q in range(n):
        assert q not in got[q]


# ---- 3. the self exclusion compares global rows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("block_rows", (10, 23, 1000))
def test_self_exclusion_uses_global_rows(sa, form, block_rows):
    pts, h = ref.duplicated_points(), ref.DUP_HALF
    run = make(sa, form, 2 * h, [0, h, 2 * h])  # both shards hold the same list of points
    try:
        with options(sa, block_rows=block_rows):
            got, dist = run.knn(pts, 3)
    finally:
        run.close()
    check(sa, pts, 3, got, dist, whole(sa, pts, 3))
    assert np.array_equal(got, oracle(pts, 3))
    # the duplicate in the other shard has the query's LOCAL row there: it is the nearest neighbour, at distance 0, and not dropped
    assert np.array_equal(got[:, 0], (np.arange(2 * h) + h) % (2 * h)) and np.all(dist[:, 0] == 0.0)


# ---- 4. the filter route ------------------------------------------------------------------------------------------------------------------
FILTER_N, FILTER_D, FILTER_K = 4096, 10, 15
FILTER_CUTS = {2: [0, 2600, 4096], 3: [0, 2500, 3100, 4096]}  # every rank has at least 256 queries and owns rows of the cluster below


def gaussian_with_duplicates():
    rng = np.random.default_rng(4096)
    pts = rng.standard_normal((FILTER_N, FILTER_D))
    src, dst = rng.permutation(FILTER_N)[:128].reshape(2, 64)
    pts[dst] = pts[src]  # 64 exact duplicate rows
    return pts


CLUSTER_ROWS = (2400, 3600)  # wholly inside the second block of 2048 rows


def gaussian_with_cluster():
    rng = np.random.default_rng(1200)
    pts = rng.standard_normal((FILTER_N, FILTER_D))
    lo, hi = CLUSTER_ROWS
    dirs = rng.standard_normal((hi - lo, FILTER_D))
    dirs *= (rng.random((hi - lo, 1)) ** (1.0 / FILTER_D)) / np.linalg.norm(dirs, axis=1, keepdims=True)
    pts[lo:hi] = pts[lo] + 1e-3 * dirs  # 1200 points inside one ball of radius 1e-3
    return pts


@pytest.fixture(scope="module")
def filter_cases(sa):
    a, b = gaussian_with_duplicates(), gaussian_with_cluster()
    return {"duplicates": (a, whole(sa, a, FILTER_K)), "cluster": (b, whole(sa, b, FILTER_K))}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shards", (2, 3))
def test_filter_route(sa, filter_cases, shards, form):
    pts, want = filter_cases["duplicates"]
    run = make(sa, form, FILTER_N, FILTER_CUTS[shards])
    try:
        with options(sa, block_rows=1024, min_points=512):
            got, dist = run.knn(pts, FILTER_K)
            st = sa.debug_knn_last_stats()
            blocks, steps = run.counters("knn_blocks"), run.counters("knn_allreduces")
    finally:
        run.close()
    check(sa, pts, FILTER_K, got, dist, want)
    assert st["filtered"] and st["rounds"] and st["rounds"][-1]["stride"] == 1 and st["rounds"][-1]["points"] == 1024
    assert blocks == [4] * shards and all(s >= 4 for s in steps)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shards", (2, 3))
def test_filter_route_overflow_is_redone_with_global_self_exclusion(sa, filter_cases, shards, form):
    pts, want = filter_cases["cluster"]
    run = make(sa, form, FILTER_N, FILTER_CUTS[shards])
    try:
        with options(sa, block_rows=2048, min_points=512):
            got, dist = run.knn(pts, FILTER_K)
            st = sa.debug_knn_last_stats()
    finally:
        run.close()
    check(sa, pts, FILTER_K, got, dist, want)
    assert st["filtered"] and [r["stride"] for r in st["rounds"]] == [2, 1]
    if form == "hook":  # (every rank of these cuts owns queries of the cluster, so whichever searched last saw lists overflow)
        assert st["rounds"][-1]["overflowed"] > 0 and st["rounds"][-1]["cand_max"] > sa.debug_knn_filter_params()["cap"]


# ---- 5. high dimension and large k ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_high_dimension_and_large_k(sa, form):
    pts = np.random.default_rng(300).standard_normal((300, 100))
    want = whole(sa, pts, 128)
    run = make(sa, form, 300, [0, 70, 200, 300])
    try:
        with options(sa, block_rows=128):
            got, dist = run.knn(pts, 128)
            assert run.counters("knn_blocks") == [3] * 3
    finally:
        run.close()
    check(sa, pts, 128, got, dist, want)


# ---- 6. the scores a PCA left on the devices ------------------------------------------------------------------------------------------
def test_device_resident_scores(sa):
    from scanrs_amd.synth import synth_counts

    m = synth_counts(2500, 500, 0.06, 12)  # cells x genes CSR = genes x cells CSC
    mm = sa.MultiMat(m.shape[1], m.shape[0], sa.CSC, m.indptr, m.indices, m.data, 2, devices=[0, 0])
    try:
        with pytest.raises(sa.ScanrsError) as e:  # 7. points=None before any PCA
            mm.knn(5)
        assert e.value.code == 6 and "no PCA result" in str(e.value)
        mm.normalize(sa.Normalization.CellRanger)
        u, s, v = mm.run_pca_bk(8)
        with options(sa, block_rows=700):
            got, dist = mm.knn(5, return_sq_dist=True)
        assert mm.counter("knn_blocks") == 4 and mm.counter("knn_blocks", shard=1) == 4
    finally:
        mm.close()
    check(sa, v, 5, got, dist, whole(sa, v, 5))


# ---- 7. refusals: every rank returns the error, nobody hangs --------------------------------------------------------------------------
def test_refusals_on_every_rank(sa):
    pts = ref.lattice_points()
    cuts = ref.LATTICE_CUTS[3]
    bad = pts.copy()
    bad[41, 1] = np.nan  # in the middle shard (rows 40, 41)
    bad[90, 0] = np.inf  # a later row of another shard: the FIRST offending global row is named
    run = Hooked(sa, cuts)
    for arg, k, text in ((bad, 5, "row 41"), (pts, 129, "k must not exceed 128"), (pts[:, :0], 5, "dimensions")):
        out = run.on_all(lambda r, h: h.knn_sharded(arg, k))
        for o in out:
            assert isinstance(o, sa.ScanrsError) and o.code == 6 and text in str(o), o
    # ranks that disagree on k
    out = run.on_all(lambda r, h: h.knn_sharded(pts, 4 if r == 1 else 5))
    for o in out:
        assert isinstance(o, sa.ScanrsError) and o.code == 6 and "disagree" in str(o), o
    got, _ = run.knn(pts, 5)  # the handles stay usable
    assert np.array_equal(got, whole(sa, pts, 5))
    mm = sa.MultiMat(1, ref.LATTICE_N, sa.CSC, *cell_matrix(ref.LATTICE_N), 3, devices=[0, 0, 0])
    try:
        for arg, k, text in ((bad, 5, "row 41"), (pts, 129, "k must not exceed 128"), (pts[:, :0], 5, "dimensions")):
            with pytest.raises(sa.ScanrsError) as e:
                mm.knn(k, arg)
            assert e.value.code == 6 and text in str(e.value)
        with pytest.raises(sa.ScanrsError) as e:
            mm.knn(5)
        assert e.value.code == 6
        assert np.array_equal(mm.knn(5, pts), whole(sa, pts, 5))
    finally:
        mm.close()


# ---- 9. an unsharded handle -----------------------------------------------------------------------------------------------------------
def test_unsharded_handle_is_plain_knn(sa):
    pts = ref.lattice_points()
    h = sa.AdaptiveMat.from_csmat(1, ref.LATTICE_N, sa.CSC, *cell_matrix(ref.LATTICE_N))
    got, dist = h.knn_sharded(pts, 5, return_sq_dist=True)
    assert np.array_equal(got, sa.knn(pts, 5))
    same_bits(dist, ref.sq_dist_pairs(pts, got))
    assert h.counter("knn_blocks") == 0 and h.counter("knn_allreduces") == 0
